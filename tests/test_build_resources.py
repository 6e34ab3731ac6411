"""The built library's kernels do not spill (CPU test: reads what `csrc/build.sh` recorded while compiling).

`hipcc -Rpass-analysis=kernel-resource-usage` prints, per kernel, its register counts, scratch bytes per lane and spill counts;
build.sh keeps that text in `arxiv_rag_amd/_build/<file>.resources.txt`.  A hot kernel that spills stores its registers to
memory once per wave: the first shipped build of the round-2 attention kernel spilled 16 registers that only its fallback path
needed — 0.4 GB of extra writes per launch, invisible to every parity test (found in the WRITE_SIZE counter pass)."""
import ctypes
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
BUILD = ROOT / "arxiv_rag_amd" / "_build"
PAT = re.compile(r"Function Name: (\S+).*?VGPRs: (\d+).*?AGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)"
                 r".*?SGPRs Spill: (\d+).*?VGPRs Spill: (\d+)", re.S)


def _kernels():
    out = {}
    for f in sorted(BUILD.glob("*.resources.txt")):
        for m in PAT.finditer(f.read_text()):
            out[m.group(1)] = dict(vgprs=int(m.group(2)), agprs=int(m.group(3)), scratch=int(m.group(4)), occupancy=int(m.group(5)),
                                   sgpr_spill=int(m.group(6)), vgpr_spill=int(m.group(7)))
    return out


def test_no_kernel_of_the_build_spills_or_uses_scratch():
    ks = _kernels()
    if not ks:
        pytest.skip("no _build/*.resources.txt (library not built by csrc/build.sh in this tree)")
    assert len(ks) > 40                                      # encoder + search + runtime kernels, all template instances
    # (SGPR spills go to lanes of a VGPR, not to memory: the persistent GEMMs have a few and that is fine)
    bad = {k: v for k, v in ks.items() if v["scratch"] or v["vgpr_spill"]}
    assert not bad, bad


def test_hot_kernels_keep_their_occupancy():
    """the occupancy each hot kernel was designed for (waves per SIMD): attention 4 (two 8-wave blocks per CU), the 256x256
    GEMMs 2 (one 8-wave block, 256 registers), search pass A >= 2"""
    ks = _kernels()
    if not ks:
        pytest.skip("no _build/*.resources.txt")
    att = {k: v for k, v in ks.items() if "attention_tr_kernel" in k and k.endswith("ELi8EEvPKtPtPKiPKfifiPy")}
    assert att and all(v["occupancy"] >= 4 for v in att.values()), att
    gemm = {k: v for k, v in ks.items() if "gemm_8phase" in k}
    assert gemm and all(v["occupancy"] >= 2 for v in gemm.values()), gemm
    srch = {k: v for k, v in ks.items() if "search_groupmax_kernel" in k}
    assert srch and all(v["occupancy"] >= 2 for v in srch.values()), srch


def test_shipped_library_does_not_import_getenv():
    """include/arx.h: the library reads no environment variable (what a handle or a search runs is in its arguments).  A dev build
    (-DARX_DEV_VARIANTS, marked by its arx_dev_attn_set export) keeps a few measurement switches and is not held to this."""
    from arxiv_rag_amd import _lib
    nm = shutil.which("nm")
    if nm is None:
        pytest.skip("no nm on this machine")
    assert _lib.LIB_PATH.exists(), "libarx_hip.so not built (run __graft_entry__.build())"
    if hasattr(ctypes.CDLL(str(_lib.LIB_PATH)), "arx_dev_attn_set"):
        pytest.skip("a dev build is loaded")
    undefined = subprocess.run([nm, "-D", "--undefined-only", str(_lib.LIB_PATH)], check=True, capture_output=True, text=True).stdout
    assert len(undefined.split()) > 20, "nm listed no imports"
    assert "getenv" not in undefined, [l for l in undefined.splitlines() if "getenv" in l]


def test_encoder_options_struct_matches_the_header():
    from arxiv_rag_amd import _lib
    body = re.search(r"typedef struct \{([^}]*)\} arx_encoder_options;", (ROOT / "include" / "arx.h").read_text()).group(1)
    fields = re.findall(r"^\s*(\w+)\s+(\w+);", body, re.M)
    assert fields and all(t == "int32_t" for t, _ in fields), fields
    assert [n for _, n in fields] == [n for n, _ in _lib.EncoderOptionsC._fields_]
    assert all(t is ctypes.c_int32 for _, t in _lib.EncoderOptionsC._fields_)
    assert ctypes.sizeof(_lib.EncoderOptionsC) == 4 * len(fields) == _lib.EncoderOptionsC().struct_bytes
    hdr = (ROOT / "include" / "arx.h").read_text()
    for name in ("GEMM_DEFAULT", "GEMM_PER_TILE", "GEMM_PERSISTENT", "GEMM_2STAGE", "GEMM_SPLIT_K", "GEMM_TILE_128", "ATTN_TRANSPOSED",
                 "ATTN_RING", "ATTN_RING16", "ATTN_STAGED", "ENC_EXPLICIT_LAYERNORM"):
        assert int(re.search(rf"#define ARX_{name}\s+(\d+)", hdr).group(1)) == getattr(_lib, name), name
