"""The option table (tensorized-rnn_amd/csrc/ttrnn_opts.h): every A/B route switch is a named 0 / 1 option, and the two words whose
bits the switches used to be — "dev", "dev2" — stay settable by number.  Pure host state: no test here needs a device.
    LEGACY is the frozen map: the 40 (word, mask) pairs as the call sites tested them before the switches had names.  It is
    a literal on purpose — a renamed or re-numbered row must fail here, not follow the table.
    SWITCHED: host-side queries that answer differently under a switch; `legacy` is what the library answered under the
    numeric mask before the change (recorded from that build on a machine without a device).
"""
import ctypes
import os
import re
import subprocess
import sys

import pytest

LEGACY = [
    ("dev", 1, "gemm3_pingpong"), ("dev", 4, "f10gq_bf16"), ("dev", 32, "gru_eight_wave"), ("dev", 64, "gemm3_wg_per_tile"),
    ("dev", 128, "f10bl_always"), ("dev", 256, "gru_fwd_on_tier"), ("dev", 512, "f10s"), ("dev", 1024, "no_proj3"),
    ("dev", 2048, "g2_bwd_head_streamed"), ("dev", 4096, "g2_four_wave_streamed"), ("dev", 8192, "h512_fwd_on_tier"),
    ("dev", 16384, "h512_bwd_on_tier"), ("dev", 32768, "f10bl_never"), ("dev", 1 << 16, "no_fused_setup"), ("dev", 1 << 17, "f10p"),
    ("dev", 1 << 18, "head_split_epilogue"), ("dev", 1 << 19, "g2_pair_never"), ("dev", 1 << 20, "g2_pair_always"),
    ("dev", 1 << 21, "g2_bwd_four_wave"), ("dev", 1 << 22, "g2_bwd_t2_general"), ("dev", 1 << 23, "no_proj4"),
    ("dev", 1 << 24, "g2_dense_from_merged"), ("dev", 1 << 25, "naive_fwd_on_tier"), ("dev", 1 << 26, "gru_r16_bwd_stagewise"),
    ("dev", 1 << 27, "g2_no_cin"), ("dev", 1 << 28, "dense_one_round_rule"), ("dev", 1 << 29, "g2_bwd_one_tile"),
    ("dev2", 1, "no_chain_wgrad"), ("dev2", 2, "chain_wgrad_hid_only"), ("dev2", 4, "c2_runtime_plan"), ("dev2", 8, "chain_wgrad_large"),
    ("dev2", 16, "enc_fwd_on_tier"), ("dev2", 32, "enc_bwd_on_tier"), ("dev2", 64, "c2r_off"), ("dev2", 128, "gru_r16_bwd_on_tier"),
    ("dev2", 256, "gru_h512_bwd_on_tier"), ("dev2", 512, "naive_bwd_on_tier"), ("dev2", 1024, "f10bh_no_wl"), ("dev2", 2048, "f10t_off"),
    ("dev2", 4096, "f10t_r7_loop"),
]
OTHERS = ["fp32_math", "force_generic", "no_gemm", "no_in1", "no_f10", "no_g2", "force_g2", "diag", "bf16_fp32_mfma", "big_merge",
          "big_no_gemm", "big_no_pair", "no_bigb", "bigw_slices", "f10_nb1", "dense_fp32", "f10_nb2", "gemm_pieces", "big_fp32_mfma",
          "pair_fault", "no_gemm3", "dev", "dev2"]
SWITCHES = [name for _, _, name in LEGACY]
UNSUPPORTED = -3      # TTRNN_ERR_UNSUPPORTED
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def opts():
    """the library's option calls, with every switch and both words at 0 before and after the test"""
    import ttrnn_hip
    for word in ("dev", "dev2"):
        ttrnn_hip.set_option(word, 0)
    yield ttrnn_hip
    for word in ("dev", "dev2"):
        ttrnn_hip.set_option(word, 0)


def _on(o):
    return [n for n in SWITCHES if o.get_option(n)]


def test_frozen_map_is_40_disjoint_masks():
    assert len(LEGACY) == 40 and len(set(SWITCHES)) == 40
    for word, count in (("dev", 27), ("dev2", 13)):
        masks = [m for w, m, _ in LEGACY if w == word]
        assert len(masks) == count and all(m & (m - 1) == 0 for m in masks)
        assert sum(masks) == (0x3FFFFFFF & ~(2 | 8 | 16) if word == "dev" else 8191)      # disjoint: the sum is the union


@pytest.mark.parametrize("word,mask,name", LEGACY, ids=SWITCHES)
def test_number_and_name_are_two_views_of_one_switch(opts, word, mask, name):
    other = "dev2" if word == "dev" else "dev"
    assert _on(opts) == [] and opts.get_option("dev") == 0 and opts.get_option("dev2") == 0
    opts.set_option(word, mask)
    assert opts.get_option(name) == 1 and _on(opts) == [name]
    opts.set_option(word, 0)
    assert _on(opts) == []
    opts.set_option(name, 1)
    assert opts.get_option(word) == mask and opts.get_option(other) == 0 and _on(opts) == [name]
    opts.set_option(name, 0)
    assert opts.get_option(word) == 0
    # the context manager restores both views, in either nesting
    with opts.option(name, 1):
        assert opts.get_option(word) == mask
        with opts.option(word, 0):
            assert opts.get_option(name) == 0
        assert opts.get_option(name) == 1 and opts.get_option(word) == mask
    assert opts.get_option(name) == 0 and opts.get_option(word) == 0
    with opts.option(word, mask):
        with opts.option(name, 0):
            assert opts.get_option(word) == 0
        assert opts.get_option(word) == mask and opts.get_option(name) == 1
    assert opts.get_option(name) == 0 and opts.get_option(word) == 0


def test_ablation_bits_survive_named_sets(opts):
    opts.set_option("dev", 2)
    opts.set_option("f10s", 1)
    assert opts.get_option("dev") == 2 | 512
    opts.set_option("f10s", 0)
    assert opts.get_option("dev") == 2
    opts.set_option("dev2", 5 << 16)
    with opts.option("f10t_off", 1):
        assert opts.get_option("dev2") == (5 << 16) | 2048
    assert opts.get_option("dev2") == 5 << 16 and _on(opts) == []
    opts.set_option("dev", 2 | 8 | 16 | 128 | 32768)
    assert _on(opts) == ["f10bl_always", "f10bl_never"] and opts.get_option("dev") == 2 | 8 | 16 | 128 | 32768


def test_bad_names_and_values_change_nothing(opts):
    from ttrnn_hip import _lib
    lib = _lib.load()
    opts.set_option("dev", 2 | 512)
    before = {n: opts.get_option(n) for n in OTHERS + SWITCHES}
    v = ctypes.c_int(77)
    assert lib.ttrnn_set_option(b"no_such_option", 1) == UNSUPPORTED
    assert lib.ttrnn_get_option(b"no_such_option", ctypes.byref(v)) == UNSUPPORTED and v.value == 77
    assert lib.ttrnn_set_option(None, 1) == UNSUPPORTED
    for name in ("f10s", "enc_fwd_on_tier", "no_f10"):
        assert lib.ttrnn_set_option(name.encode(), 2) == UNSUPPORTED and lib.ttrnn_set_option(name.encode(), -1) == UNSUPPORTED
    for word in (b"dev", b"dev2"):
        assert lib.ttrnn_set_option(word, -1) == UNSUPPORTED and lib.ttrnn_set_option(word, 0x40000000) == UNSUPPORTED
    assert lib.ttrnn_set_option(b"big_merge", 3) == UNSUPPORTED and lib.ttrnn_set_option(b"gemm_pieces", 1) == UNSUPPORTED
    assert lib.ttrnn_set_option(b"fp32_math", 2) == UNSUPPORTED
    assert {n: opts.get_option(n) for n in OTHERS + SWITCHES} == before
    assert lib.ttrnn_set_option(b"dev", 0x3FFFFFFF) == 0 and len(_on(opts)) == 27


def test_options_epoch_moves_on_a_change_only(opts):
    from ttrnn_hip import _lib
    e = _lib.OPTIONS_EPOCH
    opts.set_option("enc_fwd_on_tier", 0)
    opts.set_option("dev2", 0)
    with opts.option("f10s", 0):
        pass
    assert _lib.OPTIONS_EPOCH == e
    opts.set_option("enc_fwd_on_tier", 1)
    assert _lib.OPTIONS_EPOCH == e + 1
    opts.set_option("dev2", 16)            # the same state, by number
    assert _lib.OPTIONS_EPOCH == e + 1
    opts.set_option("dev2", 0)
    assert _lib.OPTIONS_EPOCH == e + 2


def _child(env, *names):
    """option values as a fresh process reads them from its environment (no GPU work in it)"""
    from ttrnn_hip import _lib
    code = ("import ctypes, sys\nlib, v = ctypes.CDLL(%r), ctypes.c_int()\nfor n in sys.argv[1:]:\n"
            "    assert lib.ttrnn_get_option(n.encode(), ctypes.byref(v)) == 0\n    print(v.value)" % _lib.LIB_PATH)
    e = {k: v for k, v in os.environ.items() if not k.startswith("TTRNN_")}
    e.update(env)
    out = subprocess.run([sys.executable, "-c", code] + list(names), env=e, check=True, capture_output=True, text=True).stdout
    return [int(v) for v in out.split()]


def test_environment():
    assert _child({"TTRNN_DEV2": "16"}, "enc_fwd_on_tier", "enc_bwd_on_tier", "dev2") == [1, 0, 16]
    assert _child({"TTRNN_ENC_FWD_ON_TIER": "1"}, "dev2", "dev") == [16, 0]
    assert _child({"TTRNN_DEV2": "0", "TTRNN_ENC_FWD_ON_TIER": "1"}, "enc_fwd_on_tier", "dev2") == [1, 16]      # the name wins
    assert _child({"TTRNN_DEV2": "48", "TTRNN_ENC_FWD_ON_TIER": "0"}, "enc_fwd_on_tier", "enc_bwd_on_tier", "dev2") == [0, 1, 32]
    assert _child({"TTRNN_DEV": str(2 | 512 | 1 << 29)}, "f10s", "g2_bwd_one_tile", "dev") == [1, 1, 2 | 512 | 1 << 29]
    assert _child({}, "dev", "dev2", "fp32_math", "big_merge", "gemm_pieces") == [0, 0, 1, 2, 0]
    assert _child({"TTRNN_FP32_MATH": "exact", "TTRNN_BIG_MERGE": "1", "TTRNN_GEMM_PIECES": "3", "TTRNN_NO_F10": "1"},
                  "fp32_math", "big_merge", "gemm_pieces", "no_f10") == [0, 1, 3, 1]


def test_header_lists_exactly_the_tables_names(opts):
    """include/ttrnn.h's comment above ttrnn_set_option names every option; csrc/ttrnn_opts.h's table is what the library answers to"""
    with open(os.path.join(ROOT, "include", "ttrnn.h")) as f:
        text = f.read()
    block = text[text.index("/* Library options"):text.index("int ttrnn_set_option")]
    block = block[block.index("Names (value 0 / 1 unless noted):"):]
    documented = re.findall(r'"([a-z0-9_]+)"', block)
    with open(os.path.join(ROOT, "tensorized-rnn_amd", "csrc", "ttrnn_opts.h")) as f:
        rows = re.findall(r'^\s*X\((\w+),\s*"([a-z0-9_]+)",\s*\w+,\s*\w+,\s*(\w+),\s*([^,]+),', f.read(), re.M)
    table = [name for _, name, _, _ in rows]
    assert len(set(table)) == len(table) == len(OTHERS) + 40
    assert sorted(documented) == sorted(table) == sorted(OTHERS + SWITCHES)
    assert all(ident == name.upper() for ident, name, _, _ in rows)      # OPT_<NAME> and TTRNN_<NAME> follow from the name
    assert sorted((w.lower(), eval(m), n) for _, n, w, m in rows if w != "NONE") == sorted(LEGACY)
    for name in table:
        opts.get_option(name)      # raises on a name the library does not know


# ---- the switches still switch --------------------------------------------------------------------------------------------------
def _spec(**meta):
    import torch
    from golden_io import build_module
    meta.setdefault("num_layers", 1)
    return build_module(meta, torch.device("cpu"))._all_layers[0]._layer_spec()


def _tt(kind, H, rank, **kw):
    return dict(kind=kind, input_size=1, hidden_size=H, n_cores=3, tt_rank=rank, **kw)


ENC = dict(kind="ttlstm", input_size=40, hidden_size=768, n_cores=2, tt_rank=2)
FWD, BWD = ("ttrnn_rnn_forward_route",), ("ttrnn_rnn_backward_route", 0)
# name: (module, batch, steps, query and its extra arguments, answer by default, answer under the numeric mask before the change)
SWITCHED = {
    "enc_fwd_on_tier": (ENC, 6, 11, FWD, 2, 4),
    "enc_bwd_on_tier": (ENC, 6, 11, BWD, 2, 4),
    "no_chain_wgrad": (ENC, 64, 32, ("ttrnn_rnn_wgrad_workspace", 3), None, 0),
    "f10t_off": (_tt("ttlstm", 256, 8), 64, 784, ("ttrnn_rnn_forward_cores01_first",), 1, 0),
    "no_fused_setup": (_tt("ttlstm", 256, 8), 64, 784, ("ttrnn_rnn_forward_cores_fused",), 1, 0),
    "h512_fwd_on_tier": (dict(_tt("ttlstm", 512, 8), input_size=40), 4, 9, FWD, 2, 4),      # (its kernel does not take one input)
    "h512_bwd_on_tier": (_tt("ttlstm", 512, 8), 4, 9, BWD, 2, 4),
    "naive_fwd_on_tier": (_tt("ttlstm", 256, 8, is_naive=True), 4, 9, FWD, 2, 4),
    "naive_bwd_on_tier": (_tt("ttlstm", 256, 8, is_naive=True), 4, 9, BWD, 2, 4),
    "gru_fwd_on_tier": (_tt("ttgru", 256, 8), 4, 9, FWD, 2, 4),
    "gru_r16_bwd_on_tier": (_tt("ttgru", 256, 16), 4, 9, BWD, 2, 4),
    "gru_h512_bwd_on_tier": (_tt("ttgru", 512, 8), 4, 9, BWD, 2, 4),
    "g2_pair_always": (_tt("ttlstm", 512, 8, is_naive=True), 4, 9, ("ttrnn_rnn_forward_samples_per_workgroup",), 1, 2),
}


@pytest.mark.parametrize("name", sorted(SWITCHED))
def test_switch_still_switches(opts, name):
    """a host-side query answers the same under the name as under the old mask, as it did before, and not as by default"""
    from ttrnn_hip import _lib
    meta, B, T, (fn, *extra), default, legacy = SWITCHED[name]
    word, mask = next((w, m) for w, m, n in LEGACY if n == name)
    desc = _spec(**meta).desc(B, T, _lib.TTRNN_F32)

    def ask():
        return getattr(_lib.load(), fn)(ctypes.byref(desc), *extra)

    base = ask()
    assert base == default if default is not None else base > 0
    with opts.option(name, 1):
        by_name = ask()
    with opts.option(word, mask):
        by_mask = ask()
    assert by_name == by_mask == legacy != base
    assert ask() == base
