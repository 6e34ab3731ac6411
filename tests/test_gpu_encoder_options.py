"""arx_encoder_options (include/arx.h): what a handle runs comes from the arguments of its create call and from nowhere else.
  - the environment variables that selected the schedules up to round 4 change nothing;
  - every alternative of the shipped build is honoured (agrees with the default to rounding and, where the schedule has other bits, differs);
  - a wrong struct size or an id the build does not contain is ARX_ERR_ARG naming the field, leaves *out alone and costs the next create nothing.
Model: 2 MiniLM layers (the LN-fold and explicit-LayerNorm paths diverge after one layer); lengths on both sides of the 128-token split
between 4- and 8-wave attention blocks."""
import ctypes
import dataclasses

import numpy as np
import pytest

from arxiv_rag_amd import _lib
from arxiv_rag_amd import config as C
from arxiv_rag_amd.weights import seeded_state_dict

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

CFG = dataclasses.replace(C.PRESETS["all-MiniLM-L6-v2"], layers=2)
LENS = np.array([200, 1, 129, 33, 64], np.int32)
ENV = {"ARX_LN_FOLD": "0", "ARX_ATTN_VARIANT": "0", "ARX_GEMM_VARIANT": "13", "ARX_GEMM_GLDS": "0"}

ALTERNATIVES = {"explicit-layernorm": {"ln_fold": False}, "attn-staged": {"attn_kernel": _lib.ATTN_STAGED},
                "gemm-8": {"gemm_schedule": _lib.GEMM_PER_TILE}, "gemm-9": {"gemm_schedule": _lib.GEMM_PERSISTENT},
                "gemm-13": {"gemm_schedule": _lib.GEMM_2STAGE}}
# the alternatives whose rows differed in bits from the default's on this input when the commit before this module selected them
# through the environment: the "differs from default" column of profiles/encoder_options_parity.md, minilm2 rows (GEMM 8 and 9 are
# the two halves of the default 89 and give its bits at these shapes)
DIFFERS = {"explicit-layernorm", "attn-staged", "gemm-13"}


def _cos(a, b):
    return (a * b).sum(-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1) + 1e-30)


@pytest.fixture(scope="module")
def model():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()
    sd = seeded_state_dict(CFG, seed=5, std=0.04, bias_std=0.03, ln_jitter=0.05)
    rs = np.random.RandomState(3)
    ids = np.full((len(LENS), int(LENS.max())), CFG.pad_id, np.int32)
    for r, n in enumerate(LENS):
        ids[r, :n] = rs.randint(4, CFG.vocab_size, size=int(n))
    return sd, ids


def _rows(model, **opts):
    from arxiv_rag_amd.encoder import HipEncoder
    sd, ids = model
    enc = HipEncoder(CFG, sd, max_tokens=int(LENS.sum()), max_seqs=len(LENS), **opts)
    out = enc.encode_tokens(ids, LENS).cpu().numpy()
    enc.close()
    assert out.dtype == np.float32 and np.isfinite(out).all()
    return out


@pytest.fixture(scope="module")
def default_rows(model):
    out = _rows(model)
    out.setflags(write=False)
    return out


def test_the_environment_is_ignored(model, monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    clean = _rows(model)
    for k, v in ENV.items():
        monkeypatch.setenv(k, v)
    assert np.array_equal(_rows(model), clean)


@pytest.mark.parametrize("alt", list(ALTERNATIVES))
def test_selections_are_honoured(model, default_rows, alt):
    from arxiv_rag_amd.encoder import HipEncoder
    opts = ALTERNATIVES[alt]
    got = _rows(model, **opts)
    worst = 1 - _cos(got, default_rows).min()
    same = np.array_equal(got, default_rows)
    print(f"{alt}: worst 1 - cos against the default {worst:.2e}; bits {'equal' if same else 'differ'}")
    assert worst < 3e-4, (alt, worst)                                    # the bound of test_alternative_schedules_agree
    if alt in DIFFERS:
        assert not same, (alt, "the selection was dropped: these are the default's bits")
    sd, _ = model
    enc = HipEncoder(CFG, sd, max_tokens=64, max_seqs=1, **opts)      # what was chosen can be read back
    want = {"gemm_schedule": _lib.GEMM_DEFAULT, "attn_kernel": _lib.ATTN_TRANSPOSED, "ln_fold": True, **opts}
    assert {k: getattr(enc, k) for k in want} == want
    enc.close()


def _raw_create(enc, opt):
    """arx_encoder_create_opt through raw ctypes with the weights of `enc` -> (rc, handle value, message); the out slot starts as a sentinel"""
    lib = _lib.load()
    h = ctypes.c_void_p(0x5A5A)
    rc = lib.arx_encoder_create_opt(ctypes.byref(enc._cfg_c), ctypes.byref(enc._weights_c), int(LENS.sum()), len(LENS),
                                    None if opt is None else ctypes.byref(opt), ctypes.byref(h))
    return rc, h.value, lib.arx_last_error().decode()


def test_refusals(model, default_rows):
    from arxiv_rag_amd.encoder import HipEncoder
    sd, ids = model
    dev = bool(_lib.load().arx_build_info() & 1)
    refused = [("gemm_schedule", 7), ("attn_kernel", 99), ("gemm_schedule", _lib.GEMM_SPLIT_K)]
    if not dev:
        refused += [("gemm_schedule", g) for g in (1, 2, 3, 4, 15, 33, 34)] + [("attn_kernel", _lib.ATTN_RING), ("attn_kernel", _lib.ATTN_RING16)]
    enc = HipEncoder(CFG, sd, max_tokens=int(LENS.sum()), max_seqs=len(LENS))
    for field, value in refused:
        with pytest.raises(_lib.ArxError, match=rf"rc=-1.*arx_encoder_options\.{field}={value}\b"):
            HipEncoder(CFG, sd, **{field: value})
        rc, h, msg = _raw_create(enc, _lib.EncoderOptionsC(**{field: value}))
        assert rc == -1 and h == 0x5A5A and f"{field}={value}" in msg, (field, value, rc, h, msg)
    for off in (4, -4):
        opt = _lib.EncoderOptionsC()
        opt.struct_bytes += off
        rc, h, msg = _raw_create(enc, opt)
        assert rc == -1 and h == 0x5A5A and f"struct_bytes={ctypes.sizeof(opt) + off}" in msg, (off, rc, h, msg)
    rc, h, msg = _raw_create(enc, _lib.EncoderOptionsC(flags=2))
    assert rc == -1 and h == 0x5A5A and "flags=0x2" in msg, (rc, h, msg)
    # a handle created right after the refusals runs the default kernels: through HipEncoder, and through raw ctypes with opt = NULL and
    # with an all-zero struct of the right size
    assert np.array_equal(_rows(model), default_rows)
    for opt in (None, _lib.EncoderOptionsC()):
        rc, h, msg = _raw_create(enc, opt)
        assert rc == 0 and h not in (None, 0, 0x5A5A), (rc, h, msg)
        own, enc._handle = enc._handle, ctypes.c_void_p(h)
        try:
            got = enc.encode_tokens(ids, LENS).cpu().numpy()
        finally:
            torch.cuda.synchronize()
            _lib.load().arx_encoder_destroy(enc._handle)
            enc._handle = own
        assert np.array_equal(got, default_rows), opt
    enc.close()
