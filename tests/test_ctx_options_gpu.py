"""The options of a context are that context's own: two contexts on device 0, raw calls of the C ABI, no kernel launched.
Every name dfa_ctx_set_option accepts (but the action poison_lds, and clock_probe, which allocates) reads back the default
include/dfa_hip.h documents on a fresh context; set on one context, it reads back there and leaves the other context alone --
the kernel-selection hooks wgrad_variant and train_conv_variant included, which once were globals of the process."""
import ctypes as C
import os
import re

import pytest

import dfa_amd  # noqa: F401
from dfa_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, E_NULL_PTR, E_UNSUPPORTED = 0, -3, -7

FLAGS = ["conv1_bwd_fused", "dgrad_m16", "conv1_mfma", "cae_enc1_mfma", "cae_enc_dma", "cae_dgrad_mfma", "cae_conv_stats", "cae_bwd_fold",
         "cae_enc4_wide", "cae_dec_fused", "block3_m16", "fuse_conv1", "fuse_blocks123", "persist123", "lds_pipe", "carry_a1", "phase123",
         "cls123"]                                             # 0/1 switches, all 1 by default
INTS = {"time_split": (-1, 3), "wgrad_variant": (3, 2), "train_conv_variant": (2, 1), "cnn1d_train_x3": (1, 3), "cnn1d_fused": (1, 2),
        "conv_dma": (-1, 1)}                                   # name: (documented default, another accepted value)
NOT_READ = {"poison_lds", "clock_probe"}


def _conv_dma_default():
    """-1, or what DFA_CONV_DMA=0|1 asked for before dfa_ctx_create (dfa_hip.h, "conv_dma")"""
    env = os.environ.get("DFA_CONV_DMA", "")
    return int(env[0]) if env[:1] in ("0", "1") else -1


def _defaults():
    d = {name: 1 for name in FLAGS}
    d.update({name: dflt for name, (dflt, _) in INTS.items()})
    d["conv_dma"] = _conv_dma_default()
    return d


class _Ctx:
    def __init__(self, lib):
        self.lib, self.h = lib, C.c_void_p()
        assert lib.dfa_ctx_create(0, None, C.byref(self.h)) == OK and self.h.value

    def set(self, name, value):
        return self.lib.dfa_ctx_set_option(self.h, name.encode(), value)

    def get(self, name):
        v = C.c_int(-12345)
        rc = self.lib.dfa_ctx_get_option(self.h, name.encode(), C.byref(v))
        return rc, v.value

    def close(self):
        if self.h.value:
            assert self.lib.dfa_ctx_destroy(self.h) == OK
            self.h = C.c_void_p()


def test_the_table_names_every_documented_option():
    header = open(os.path.join(ROOT, "include", "dfa_hip.h")).read()
    doc = header[header.index("tuning / test switches"):header.index("int dfa_ctx_set_option")]
    documented = set(re.findall(r'^ \*   "([a-z0-9_]+)"', doc, flags=re.M))
    assert documented == set(FLAGS) | set(INTS) | NOT_READ, documented ^ (set(FLAGS) | set(INTS) | NOT_READ)


def test_options_are_read_back_per_context():
    lib = _lib.load()
    a, b = _Ctx(lib), _Ctx(lib)
    try:
        defaults = _defaults()
        for ctx in (a, b):                                     # fresh contexts: the documented defaults
            for name, want in defaults.items():
                assert ctx.get(name) == (OK, want), name
        changed = {}
        for name in FLAGS:
            assert a.set(name, 0) == OK and a.get(name) == (OK, 0), name
            assert a.set(name, 7) == OK and a.get(name) == (OK, 1), name      # any non-zero value of a switch is 1
            assert a.set(name, 0) == OK
            changed[name] = 0
        for name, (_, other) in INTS.items():
            value = other if other != defaults[name] else 0
            assert a.set(name, value) == OK, name
            changed[name] = value
        for name, want in changed.items():                     # A holds what was set, every name at once ...
            assert want != defaults[name], name
            assert a.get(name) == (OK, want), name
        for name, want in defaults.items():                    # ... and B still holds every default
            assert b.get(name) == (OK, want), name
        # what is not an option with a value: unknown names, the action
        for name in ("no_such_option", "", "poison_lds"):
            rc, v = a.get(name)
            assert rc == E_UNSUPPORTED and v == -12345, name
        v = C.c_int(0)
        assert lib.dfa_ctx_get_option(None, b"time_split", C.byref(v)) == E_NULL_PTR
        assert lib.dfa_ctx_get_option(a.h, None, C.byref(v)) == E_NULL_PTR
        assert lib.dfa_ctx_get_option(a.h, b"time_split", None) == E_NULL_PTR
        assert lib.dfa_error_name(E_UNSUPPORTED) == b"DFA_E_UNSUPPORTED" and lib.dfa_error_name(E_NULL_PTR) == b"DFA_E_NULL_PTR"
    finally:
        a.close()
        b.close()
