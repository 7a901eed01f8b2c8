"""masr_amd/pass_plan.py: how predict_batch cuts a length-sorted list into device passes and how it pipelines them.  Pure functions:
no GPU, no torch."""
import importlib.util
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load():
    """the module by its file: importing the ``masr_amd`` package is not needed for it (and nothing here may need torch)"""
    spec = importlib.util.spec_from_file_location('_pass_plan_under_test', os.path.join(ROOT, 'masr_amd', 'pass_plan.py'))
    mod = importlib.util.module_from_spec(spec)
    before = set(sys.modules)
    spec.loader.exec_module(mod)
    assert not any(m == 'torch' or m.startswith('torch.') for m in set(sys.modules) - before), 'pass_plan imports torch'
    return mod


pp = _load()
HINTS = [1000, 2000, 3000, 4000, 6000, 8000, 9000, 16000]            # ascending, as _run_sorted hands them over


def test_pass_cuts_explicit_list_counts_from_the_longest_and_repeats_the_last_size():
    assert pp.pass_cuts(8, HINTS, [3, 2]) == [(0, 1), (1, 3), (3, 5), (5, 8)]


def test_pass_cuts_number_zero_empty_list_and_balanced():
    assert pp.pass_cuts(8, HINTS, 3) == [(0, 3), (3, 6), (6, 8)]
    assert pp.pass_cuts(8, HINTS, 0) == [(0, 8)]
    with pytest.raises(ValueError, match='batch_size: an empty list of pass sizes'):
        pp.pass_cuts(8, HINTS, [])
    for budget in (16000.0, 20000.0, 1.0, 1e9):
        assert pp.pass_cuts(8, HINTS, ('balanced', budget)) == pp.balanced_cuts(HINTS, budget)
    assert pp.pass_cuts(8, HINTS, ('balanced', 20000.0)) == [(0, 2), (2, 5), (5, 7), (7, 8)]


@pytest.mark.parametrize('n', [0, 1, 7])
@pytest.mark.parametrize('batch_size', [0, 1, 3, 7, 8, [3, 2], [1], [100], [2, 0], ('balanced', 5000.0), ('balanced', 0.0),
                                        ('balanced', 1e9)])
def test_pass_cuts_are_ascending_disjoint_and_cover_the_list(n, batch_size):
    cuts = pp.pass_cuts(n, HINTS[:n], batch_size)
    assert all(lo < hi for lo, hi in cuts)
    assert [lo for lo, _ in cuts] == [0] * bool(n) + [hi for _, hi in cuts[:-1]]            # each range starts where the last ended
    assert (cuts[-1][1] if cuts else 0) == n


def test_balanced_cuts_stays_importable_from_predict():
    from masr_amd import pass_plan, predict
    assert predict.balanced_cuts is pass_plan.balanced_cuts


class _Beam:
    def __init__(self, use_gpu_search, supported):
        self.use_gpu_search, self._supported = use_gpu_search, supported

    def gpu_search_supported(self, T, V):
        assert (T, V) == (1, 4233)
        return self._supported


def test_search_on_gpu_needs_a_beam_decoder_its_switch_and_its_limits():
    assert pp.search_on_gpu(_Beam(True, True), 4233) is True
    assert pp.search_on_gpu(_Beam(True, False), 4233) is False             # word-based scorer / beyond the kernel's LDS
    assert pp.search_on_gpu(_Beam(False, True), 4233) is False
    assert pp.search_on_gpu(None, 4233) is False                           # another decoder


@pytest.mark.parametrize('decoder, gpu_search, env, reverse, depth, lanes', [
    ('ctc_greedy', False, {}, False, 2, 2),
    ('attention_rescoring', False, {}, False, 2, 2),
    ('attention', False, {}, False, 2, 2),
    ('ctc_beam_search', False, {}, True, 3, 2),                                          # host threads, deferred
    ('ctc_beam_search', False, {'MASR_HOST_SEARCH_DEFER': '0'}, False, 2, 2),
    ('ctc_beam_search', True, {}, True, 4, 1),
    ('ctc_beam_search', True, {'MASR_LANES': '2'}, True, 4, 2),
    ('ctc_beam_search', True, {'MASR_LANES': '7'}, True, 4, 2),                         # clamped
    ('ctc_greedy', False, {'MASR_LANES': '7'}, False, 2, 2),
    ('ctc_greedy', False, {'MASR_LANES': '0'}, False, 2, 1),
    ('ctc_greedy', False, {'MASR_LANES': '1'}, False, 2, 1),
])
def test_pass_policy(decoder, gpu_search, env, reverse, depth, lanes):
    plan = pp.pass_policy(decoder, gpu_search, 3, env)
    assert (plan.reverse, plan.depth, plan.lanes) == (reverse, depth, lanes)
    assert plan.prep_ahead is (lanes > 1)                                  # on by default wherever there is a second lane
    assert pp.pass_policy(decoder, gpu_search, 3, dict(env, MASR_PREP_AHEAD='0')).prep_ahead is False
    # one pass: one lane whatever the decoder and the environment, nothing to prepare ahead; ordering and depth as above
    one = pp.pass_policy(decoder, gpu_search, 1, env)
    assert (one.reverse, one.depth, one.lanes, one.prep_ahead) == (reverse, depth, 1, False)
