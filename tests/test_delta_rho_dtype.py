"""CPU: the opt-in float32 ``delta_rho`` (MLX_FLAG_DRHO_F32, ABI version 9) -- the flag in the
header, the binding and the library; the argument checks it changes, with fake pointers that no
check dereferences (as tests/test_abi.py); and the switch that decides the field's dtype
(momlevel_amd.steric.delta_rho_dtype_for), which is pure host logic.  The arithmetic is on the GPU:
tests/test_gpu_delta_rho_f32.py.
"""

import ctypes
import os
import re

import pytest

from momlevel_amd import _lib
from momlevel_amd.steric import delta_rho_dtype_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "momlevel_hip.h")

E_SHAPE, E_ENUM, E_ALIGN = -2, -3, -5
FAKE = 1 << 20  # 16-byte aligned, non-NULL, never dereferenced by an argument check
NEG_INV = -1.0 / 1035.0


def _local(flags, delta_rho_out, nt=2, nz=3, plane=32):
    n3 = nz * plane
    return _lib.load().mlx_steric_local(
        FAKE, FAKE, _lib.DTYPE_F64, FAKE, FAKE, FAKE, None, None, FAKE, _lib.P_ZPROF,
        _lib.EOS_WRIGHT, NEG_INV, nt, nz, plane, n3, n3, flags, delta_rho_out, FAKE, None)


def _decomp(flags, delta_rho_out, vstride, nt=2, nz=3, plane=32):
    n3 = nz * plane
    return _lib.load().mlx_steric_local_decomp(
        FAKE, FAKE, FAKE, FAKE, _lib.DTYPE_F64, FAKE, FAKE, FAKE, None, None, FAKE, _lib.P_ZPROF,
        _lib.EOS_WRIGHT, NEG_INV, nt, nz, plane, n3, n3, flags, delta_rho_out, vstride, FAKE,
        nt * plane, None)


def test_flag_and_version_agree_everywhere():
    text = open(HEADER).read()
    assert re.search(r"^#define MLX_FLAG_DRHO_F32 4\b", text, flags=re.M)
    assert int(re.search(r"#define MLX_ABI_VERSION (\d+)", text).group(1)) == 9
    assert _lib.FLAG_DRHO_F32 == 4
    assert _lib.ABI_VERSION == 9
    assert ctypes.CDLL(_lib.LIB_PATH).mlx_version() == 9
    # the flag shares no bit with the others
    assert _lib.FLAG_DRHO_F32 & (_lib.FLAG_SKIP_DRY | _lib.FLAG_FMA | 0xFF00) == 0


# More time blocks than a grid holds ("nt too large for one call: chunk it", MLX_E_SHAPE) is the
# LAST argument check of K2, behind the alignment checks, and it launches nothing: a call that
# returns it has passed them, on a box with a GPU as on one without.
NT_TOO_LARGE = 65536 * 64


def test_float32_delta_rho_needs_only_4_byte_alignment():
    odd = FAKE + 4  # 4- but not 8-byte aligned
    assert _local(0, odd) == E_ALIGN
    assert "8-byte" in _lib.last_error()
    assert _local(_lib.FLAG_SKIP_DRY, odd) == E_ALIGN
    # with the flag the same pointer passes every alignment check ...
    assert _local(_lib.FLAG_DRHO_F32, odd, nt=NT_TOO_LARGE) == E_SHAPE
    assert "nt too large" in _lib.last_error()
    # ... but a float32 element still has an alignment of its own
    assert _local(_lib.FLAG_DRHO_F32, FAKE + 2) == E_ALIGN
    assert "4-byte" in _lib.last_error()
    # without a delta_rho output the flag is ignored, not refused
    assert _local(_lib.FLAG_DRHO_F32, None, nt=NT_TOO_LARGE) == E_SHAPE
    assert "nt too large" in _lib.last_error()


def test_float32_delta_rho_call_gets_past_the_argument_checks():
    """with the flag, the 4-byte-aligned output reaches the launch: a positive hipError_t in a
    process without a device (fake pointers: GPU-less processes only, as the ABI fuzzer)"""
    import torch

    if torch.cuda.is_available():
        pytest.skip("fake pointers reach a launch: GPU-less processes only")
    assert _local(_lib.FLAG_DRHO_F32, FAKE + 4) > 0
    assert _local(_lib.FLAG_DRHO_F32 | _lib.FLAG_SKIP_DRY, FAKE) > 0
    assert _decomp(_lib.FLAG_DRHO_F32, FAKE + 4, 2 * 3 * 32) > 0


def test_other_entry_points_refuse_the_flag():
    lib = _lib.load()
    rc = lib.mlx_steric_global(FAKE, FAKE, 0, FAKE, FAKE, _lib.P_ZPROF, _lib.EOS_WRIGHT, 2, 3, 32,
                               96, 96, _lib.FLAG_DRHO_F32, FAKE, FAKE, 1 << 20, None)
    assert rc == E_ENUM and "flag" in _lib.last_error()
    rc = lib.mlx_steric_global_decomp(FAKE, FAKE, FAKE, FAKE, 0, FAKE, FAKE, _lib.P_ZPROF,
                                      _lib.EOS_WRIGHT, 2, 3, 32, 96, 96, _lib.FLAG_DRHO_F32, FAKE,
                                      FAKE, 1 << 20, None)
    assert rc == E_ENUM
    rc = lib.mlx_eos_map(FAKE, FAKE, 0, FAKE, _lib.P_ZPROF, _lib.EOS_WRIGHT, _lib.FUNC_DENSITY, 2, 3,
                         32, 96, 96, _lib.FLAG_DRHO_F32, FAKE, None)
    assert rc == E_ENUM
    # K2 still refuses bits it does not know
    assert _local(8, FAKE) == E_ENUM
    assert _local(_lib.FLAG_DRHO_F32 | 8, FAKE) == E_ENUM


def test_decomp_variant_stride_counts_float32_elements():
    nt, nz, plane = 2, 3, 32
    n4 = nt * nz * plane
    for flags in (0, _lib.FLAG_DRHO_F32):
        assert _decomp(flags, FAKE, n4 - 1) == E_SHAPE
        assert "variant strides" in _lib.last_error()
    # a stride of exactly one float32 field is enough (half the BYTES of a float64 field's)
    assert _decomp(_lib.FLAG_DRHO_F32, FAKE + 4, n4, nt=NT_TOO_LARGE) == E_SHAPE
    assert "variant strides" in _lib.last_error()  # (n4 of the longer record: still too short)
    big = NT_TOO_LARGE * nz * plane
    assert _decomp(_lib.FLAG_DRHO_F32, FAKE + 4, big, nt=NT_TOO_LARGE) == E_SHAPE
    assert "nt too large" in _lib.last_error()
    assert _decomp(0, FAKE + 4, big, nt=NT_TOO_LARGE) == E_ALIGN


def test_switch_default_is_float64():
    assert delta_rho_dtype_for("float32", environ={}) == "float64"
    assert delta_rho_dtype_for("float64", environ={}) == "float64"
    assert delta_rho_dtype_for("float32", environ={"MOMLEVEL_AMD_DELTA_RHO_DTYPE": "float64"}) == "float64"


def test_switch_follows_the_encoding():
    env = {"MOMLEVEL_AMD_DELTA_RHO_DTYPE": "encoding"}
    assert delta_rho_dtype_for("float32", environ=env) == "float32"
    assert delta_rho_dtype_for("float64", environ=env) == "float64"
    assert delta_rho_dtype_for("f4", environ=env) == "float32"
    assert delta_rho_dtype_for("int16", environ=env) == "float64"  # anything else stays float64
    assert delta_rho_dtype_for("no such dtype", environ=env) == "float64"
    assert delta_rho_dtype_for("float32", "encoding", environ={}) == "float32"
    assert delta_rho_dtype_for("float64", "encoding", environ={}) == "float64"


def test_keyword_beats_environment():
    env = {"MOMLEVEL_AMD_DELTA_RHO_DTYPE": "encoding"}
    assert delta_rho_dtype_for("float32", "float64", environ=env) == "float64"
    assert delta_rho_dtype_for("float32", "encoding",
                               environ={"MOMLEVEL_AMD_DELTA_RHO_DTYPE": "float64"}) == "float32"
    # ... also over a junk environment value: the keyword is the one that is read
    assert delta_rho_dtype_for("float32", "encoding",
                               environ={"MOMLEVEL_AMD_DELTA_RHO_DTYPE": "junk"}) == "float32"


def test_switch_reads_the_process_environment(monkeypatch):
    monkeypatch.delenv("MOMLEVEL_AMD_DELTA_RHO_DTYPE", raising=False)
    assert delta_rho_dtype_for("float32") == "float64"
    monkeypatch.setenv("MOMLEVEL_AMD_DELTA_RHO_DTYPE", "encoding")
    assert delta_rho_dtype_for("float32") == "float32"


@pytest.mark.parametrize("junk", ["float32", "f32", "", "Encoding", "1"])
def test_switch_refuses_unknown_values(junk):
    with pytest.raises(ValueError, match="'float64', 'encoding'"):
        delta_rho_dtype_for("float32", environ={"MOMLEVEL_AMD_DELTA_RHO_DTYPE": junk})
    with pytest.raises(ValueError, match="delta_rho_dtype must be one of"):
        delta_rho_dtype_for("float32", junk, environ={})


def test_core_dtype_argument():
    import torch

    from momlevel_amd import core

    assert core._delta_rho_dtype(None) == torch.float64
    assert core._delta_rho_dtype(torch.float64) == torch.float64
    assert core._delta_rho_dtype(torch.float32) == torch.float32
    for bad in (torch.float16, "float32", 4):
        with pytest.raises(ValueError):
            core._delta_rho_dtype(bad)
