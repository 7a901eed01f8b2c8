"""CPU: masr_amd.build refuses a source list that names a file csrc/ does not hold.

The engine's host code is in more than one file (engine.hip, engine_layers.hip, one file per model family -- engine_conformer.hip,
engine_efficient.hip, engine_squeezeformer.hip, engine_ds2.hip --, engine_ctc.hip, engine_frontend.hip, engine_ops.hip,
engine_attdecoder.hip; map: csrc/engine_state.h; the encoders' shared declarations: csrc/engine_encoder.h).  A listed file that
is missing used to be dropped without a word: the link then lacked its object, and the library loaded and died in the first call that
reached a function of it.  Nothing here compiles, and neither the source tree nor the library is touched: the check runs on a copy
of the list.
"""
import os

import pytest

from masr_amd import build


def test_every_listed_source_is_in_csrc():
    listed = [s for s in build.SOURCES if s not in build.EXPERIMENT_SOURCES]
    assert build._sources(listed) == listed
    # and the other way round: every translation unit of the engine that csrc/ holds is listed, with the header they share
    engine_units = sorted(f for f in os.listdir(build.CSRC) if f.startswith('engine') and f.endswith('.hip'))
    assert 'engine.hip' in engine_units and set(engine_units) <= set(listed)
    assert os.path.join(build.CSRC, 'engine_state.h') in build.HEADERS
    assert os.path.join(build.CSRC, 'engine_encoder.h') in build.HEADERS


def test_a_listed_source_that_is_missing_is_an_error():
    ghost = 'engine_no_such_family.hip'
    assert not os.path.exists(os.path.join(build.CSRC, ghost))
    before = list(build.SOURCES)
    with pytest.raises(FileNotFoundError, match=ghost):
        build._sources(before + [ghost])
    assert build.SOURCES == before                 # the real list is as it was


def test_a_missing_experiment_source_is_still_tolerated(monkeypatch):
    ghost = 'ffn_no_such_experiment.hip'
    assert not os.path.exists(os.path.join(build.CSRC, ghost))
    listed = [s for s in build.SOURCES if s not in build.EXPERIMENT_SOURCES]
    monkeypatch.setattr(build, 'EXPERIMENT_SOURCES', build.EXPERIMENT_SOURCES + [ghost])
    assert build._sources(listed + [ghost]) == listed
