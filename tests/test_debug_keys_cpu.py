"""CPU: the table of process-wide masr_debug_set switches (masr_amd/csrc/knobs.h) as masr_debug_key_info lists it -- key numbers,
names, defaults and the experimental marks are part of the interface (bench.py, tools/studies and MASR_AB strings use the numbers)
-- and the state lives in that one struct: every field is read somewhere, and no file keeps a switch of its own."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'masr_amd', 'csrc')

# (key, name, default, experimental)
TABLE = [
    (1, 'ffn_variant', 0, False),
    (5, 'no_chain', 0, False),
    (6, 'rowgemm_small', 1, False),
    (7, 'attention_fewq', 1, False),
    (8, 'no_ffn_tail', 0, False),
    (9, 'no_ffn_head', 0, False),
    (12, 'rowgemm_small_blocks', 112, False),
    (13, 'ffn_split_blocks', 192, False),
    (14, 'attention_fold', 1, False),
    (15, 'embed_split', 1, False),
    (17, 'gemm_waves', 8, False),
    (18, 'conv1_nt', 1, False),
    (19, 'hot_weights', 0, False),
    (20, 'bf16x3', 0, True),
    (21, 'gemm_bf16x3_waves', 8, True),
    (22, 'ffn_x3_rotation', 1, True),
    (23, 'ffn_packed', 2, False),
    (24, 'ffn_dual', 0, True),
    (25, 'rowgemm_packed', 1, False),
    (26, 'attention_grouped_fold', 1, False),
    (27, 'ctc_fused_blocks', 160, False),
    (28, 'attention_fewq_wgs', 48, False),
    (29, 'few_rows_path', 1, False),
    (30, 'split_head', 0, True),
    (31, 'efficient_fused', 1, False),
    (32, 'beam_lm_cache', 1, False),
    (33, 'conv2_mid_fill', 50, False),
    (34, 'attn_chain', 0, True),
    (35, 'ffn_coop', 0, True),
    (36, 'sqz_fused_blocks', 128, False),
    (37, 'beam_narrow', 1, False),
    (39, 'ffn16', 1, False),
    (40, 'conv2_rows', 1, False),
    (41, 'conv1_fused', 1, False),
    (42, 'embed_rows', 1, False),
    (43, 'rnn_mfma_units', 8, False),
]


def _sources():
    """csrc file name -> text, knobs.* left out"""
    return {os.path.basename(p): open(p).read() for p in sorted(glob.glob(os.path.join(CSRC, '*')))
            if os.path.isfile(p) and not os.path.basename(p).startswith('knobs.')}


def test_key_table_is_the_documented_one(built_lib):
    from masr_amd import _lib
    rows = _lib.debug_key_table()
    assert rows == TABLE
    assert len({r[0] for r in rows}) == len(rows) and len({r[1] for r in rows}) == len(rows)
    assert not {r[0] for r in rows} & set(_lib._ENGINE_KEYS.values())           # 2, 16, 38 stay per engine
    assert not {r[1] for r in rows} & set(_lib._ENGINE_KEYS)
    assert _lib.lib().masr_debug_key_info(len(rows), None, None, None, None) != 0
    assert _lib.lib().masr_debug_key_info(-1, None, None, None, None) != 0


def test_every_switch_is_read_by_a_launcher():
    src = _sources()
    for _, name, _, _ in TABLE:
        pat = re.compile(r'knobs\(\)\.%s\b' % name)
        assert any(pat.search(text) for text in src.values()), f'knobs().{name} is read nowhere in csrc'


def test_no_switch_keeps_state_of_its_own():
    for fname, text in _sources().items():
        for pat in (r'\bset_[a-z0-9_]+\s*\(\s*int\b', r'\bstatic\s+(?:int|bool)\s+g_'):
            found = [m.group(0) for m in re.finditer(pat, text)]
            assert not found, f'{fname}: {found}'
