"""CPU: DeepSpeech2 with ``encoder_conf.use_gru`` (deepspeech2/encoder.py:21-33) up to the engine's door.

* the encoder_conf check refuses values it does not implement and a checkpoint whose recurrent cell disagrees with the config;
* the synthetic GRU checkpoint has exactly the reference model's keys and shapes, and ``use_gru=False`` leaves the LSTM draws
  (which every existing DeepSpeech2 fixture depends on) bit for bit as they were;
* the packed artefact carries the GRU keys through.
"""
import json
import os

import pytest
import torch

from masr_amd import _lib
from masr_amd.engine import _validate_encoder_conf
from masr_amd.utils import synthetic
from oracle import shims

needs_ref = pytest.mark.skipif(not shims.reference_available(), reason='reference checkout not present')


def _small(use_gru, bidirectional=True):
    return synthetic.deepspeech2_state_dict(0, 50, rnn_size=64, num_rnn_layers=2, bidirectional=bidirectional, use_gru=use_gru)


def test_use_gru_values_are_checked():
    sd = _small(True)
    with pytest.raises(_lib.MasrError, match='use_gru'):
        _validate_encoder_conf('deepspeech2', {'use_gru': 'yes'}, sd)
    _validate_encoder_conf('deepspeech2', {'use_gru': True}, sd)
    _validate_encoder_conf('deepspeech2', {'use_gru': False}, _small(False))
    _validate_encoder_conf('deepspeech2', {}, _small(False))           # the shipped default is the LSTM
    _validate_encoder_conf('deepspeech2', {'use_gru': True}, None)      # a weight-less engine has nothing to compare


@pytest.mark.parametrize('conf_gru', [False, True])
def test_cell_mismatch_is_refused(conf_gru):
    # a GRU checkpoint under use_gru: False, and an LSTM checkpoint under use_gru: True (the reference cannot load either)
    with pytest.raises(_lib.MasrError, match='use_gru') as e:
        _validate_encoder_conf('deepspeech2', {'use_gru': conf_gru}, _small(not conf_gru))
    assert ('GRU' if not conf_gru else 'LSTM') in str(e.value)


def test_gru_state_dict_layout():
    sd = _small(True)
    H, f2 = 64, ((80 - 1) // 2 - 1) // 2
    for i, kin in ((0, 32 * f2), (1, 2 * H)):
        for suf in ('', '_reverse'):
            p = f'encoder.rnns.{i}.rnn.rnn.'
            assert tuple(sd[p + 'weight_ih_l0' + suf].shape) == (3 * H, kin)
            assert tuple(sd[p + 'weight_hh_l0' + suf].shape) == (3 * H, H)
            assert tuple(sd[p + 'bias_ih_l0' + suf].shape) == (3 * H,)
            assert tuple(sd[p + 'bias_hh_l0' + suf].shape) == (3 * H,)
        assert tuple(sd[f'encoder.rnns.{i}.layer_norm.weight'].shape) == (2 * H,)
    assert not any(k.startswith('encoder.rnns.0.rnn.weight') for k in sd)
    uni = _small(True, bidirectional=False)
    assert not any(k.endswith('_reverse') for k in uni)


@needs_ref
@pytest.mark.parametrize('streaming', [False, True])
def test_gru_state_dict_matches_reference_model(tmp_path, streaming):
    shims.install()
    from masr.model_utils.deepspeech2.model import DeepSpeech2Model
    sd = synthetic.deepspeech2_state_dict(0, 50, rnn_size=64, num_rnn_layers=3, bidirectional=not streaming, use_gru=True)
    p = os.path.join(tmp_path, 'mean_istd.json')
    json.dump({'mean': sd['encoder.global_cmvn.mean'].tolist(), 'istd': sd['encoder.global_cmvn.istd'].tolist(),
               'feature_method': 'fbank'}, open(p, 'w'))
    m = DeepSpeech2Model(input_dim=80, vocab_size=50, mean_istd_path=p, streaming=streaming,
                         encoder_conf={'num_rnn_layers': 3, 'rnn_size': 64, 'use_gru': True}, decoder_conf={'dropout_rate': 0.1})
    want = m.state_dict()
    assert set(sd) == set(want)
    for k, v in want.items():
        assert tuple(sd[k].shape) == tuple(v.shape), k
    m.load_state_dict(sd)                     # strict


def test_lstm_draws_are_unchanged():
    for bi in (True, False):
        a = synthetic.deepspeech2_state_dict(0, 50, rnn_size=64, num_rnn_layers=2, bidirectional=bi)
        b = synthetic.deepspeech2_state_dict(0, 50, rnn_size=64, num_rnn_layers=2, bidirectional=bi, use_gru=False)
        assert list(a) == list(b)
        for k in a:
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k


def test_packed_artefact_round_trips_gru(tmp_path):
    from masr_amd.infer_utils.inference_predictor import load_state_dict
    from masr_amd.utils import packed
    sd = _small(True)
    path = os.path.join(tmp_path, 'ds2_gru.masr')
    assert packed.export_packed(sd, path) == len(sd)
    back = load_state_dict(path)
    assert set(back) == set(sd) and 'encoder.rnns.1.rnn.rnn.weight_hh_l0_reverse' in back
    for k, v in back.items():
        assert torch.equal(v, sd[k].float()), k
    # and the loaded checkpoint passes the same cell check as the original
    _validate_encoder_conf('deepspeech2', {'use_gru': True}, back)
    with pytest.raises(_lib.MasrError, match='use_gru'):
        _validate_encoder_conf('deepspeech2', {'use_gru': False}, back)
