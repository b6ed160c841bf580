"""Array-level API: the HIP kernels on torch device tensors.

torch is used only as the device-array container (allocation, streams); every
number is produced by libmomlevel_hip.so.  All functions enqueue on torch's
current stream OF THE DEVICE THAT OWNS THE OPERANDS (which need not be torch's current
device) and return device tensors without synchronising.

Layout: ``(time, z_l, yh, xh)`` C-contiguous, x fastest.  A
``(z_l, yh, xh)`` tensor passed where a 4-D field is expected is broadcast over
time (the held field of the thermosteric / halosteric variants).
"""

import numpy as np
import torch

from . import _lib, hostio
from ._lib import (
    DTYPE_F32,
    DTYPE_F32_UPCAST,
    DTYPE_F64,
    DTYPE_T32_S64,
    DTYPE_T64_S32,
    EOS_IDS,
    FUNC_IDS,
    P_FULL3D,
    P_FULL4D,
    P_SCALAR,
    P_ZPROF,
    MomlevelHipError,
)

F32_MODES = {"faithful": DTYPE_F32, "upcast": DTYPE_F32_UPCAST}
# K1's default time steps per block (csrc/momlevel_hip.hip kTChunk / kTChunkHeld; reported by
# bench.py, kept in step by tests/test_host_logic.py)
K1_TCHUNK = {"steric": 32, "held": 64}
ARITH_FLAGS = {"exact": 0, "fused": _lib.FLAG_FMA}


def arith_default(kernel="k0", dtype=None):
    """Arithmetic of the Wright density when the caller does not choose (``arith=None``).

    "exact": numpy's operator-for-operator evaluation, bit-identical to the reference.
    "fused": MLX_FLAG_FMA -- contracted multiply-adds and a refined hardware reciprocal: on float64 theta/S the
    whole expression (<= 2 ulp from numpy on rho, two thirds of the VALU work per cell); on float32
    theta/S in numpy's mixed precision (``f32_mode="faithful"``) the float32 polynomial is kept
    exactly as numpy rounds it and only the float64 tail is fused (a few float64 ulp from numpy's
    own value on float32 input); with ``f32_mode="upcast"`` it is float64 arithmetic on the
    float32 values.  Parity gate either way: 1e-10 relative.

    Default policy (MOMLEVEL_AMD_ARITH unset):
      * K1, the global sums (``domain="global"``: masso(t), src/momlevel/steric.py:134-147) ->
        "fused".  No global result was ever bit-identical to numpy -- the order of summation over
        (z,y,x) already differs at the 1e-15 level -- so exact arithmetic bought nothing there and
        kept the held-field variants, the one-pass decomposition and every float32 sum on the fp64
        VALU bound.  masso(t=0) == masso0 and steric[t=0] == 0.0 hold exactly in this mode too (one
        expression tree in every kernel).
      * K0 / K2, the pointwise outputs (rho, delta_rho, local eta) -> "exact": those ARE
        bit-identical to numpy and stay so.
    MOMLEVEL_AMD_ARITH=exact|fused overrides the policy for every kernel and dtype.
    """
    import os

    mode = os.environ.get("MOMLEVEL_AMD_ARITH")
    if mode is None:
        return "fused" if kernel == "k1" else "exact"
    if mode not in ARITH_FLAGS:
        raise ValueError(f"MOMLEVEL_AMD_ARITH must be 'exact' or 'fused', got '{mode}'")
    return mode


def _arith_flag(arith, kernel="k0", dtype=None):
    """``dtype``: the MLX_DTYPE_* code of the launch (or a torch dtype).  theta and salinity of
    different dtypes have exact kernels only: the default policy and MOMLEVEL_AMD_ARITH fall back to
    "exact" there, an explicit arith="fused" is an error."""
    if dtype in (DTYPE_T32_S64, DTYPE_T64_S32):
        if arith == "fused":
            raise ValueError("arith='fused' is not available for thetao / so of different dtypes")
        return 0
    if arith is None:
        arith = arith_default(kernel, dtype)
    try:
        return ARITH_FLAGS[arith]
    except KeyError:
        raise ValueError(f"arith must be 'exact' or 'fused', got '{arith}'") from None


def require_device():
    """The product path needs the HIP library AND a GPU; fail loudly otherwise."""
    _lib.load()
    if not torch.cuda.is_available():
        raise MomlevelHipError(
            "no HIP device visible: momlevel_amd computes on MI355X only (no CPU fallback)"
        )


def _stream(device):
    """Raw hipStream_t of torch's current stream ON ``device`` (not on the current device: the
    operands may live on another GPU of the node)."""
    return torch.cuda.current_stream(device).cuda_stream


def _on(device):
    """Context for a launch: kernels are enqueued with ``device`` current, so that the library's
    hipLaunchKernelGGL targets the GPU that owns the operands whatever torch's current device is."""
    return torch.cuda.device(device)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _call(lib, name, device, *args):
    """One launch of the C ABI: ``lib.<name>(*args, stream)`` on torch's current stream of
    ``device``, with ``device`` current; a non-zero status raises ``MomlevelHipError``."""
    with _on(device):
        rc = getattr(lib, name)(*args, _stream(device))
    _lib.check(rc, name)


def _float_code(x, name, ndim=None):
    """The dtype code of an operand the kernels read in place: a contiguous (``ndim``-D, when
    given) float32 or float64 device tensor."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda):
        raise TypeError(f"{name} must be a device tensor")
    if x.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"{name} must be float32 or float64, got {x.dtype}")
    if (ndim is not None and x.dim() != ndim) or not x.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {ndim}-D tensor" if ndim is not None
                         else f"{name} must be contiguous")
    return DTYPE_F64 if x.dtype == torch.float64 else DTYPE_F32


def _query_dtype(dtype):
    """The dtype code of a geometry query's ``dtype`` (a torch or numpy float32 / float64)."""
    name = str(dtype).replace("torch.", "")
    name = name if name in ("float32", "float64") else np.dtype(dtype).name
    if name not in ("float32", "float64"):
        raise TypeError(f"records are float32 or float64, not {name}")
    return DTYPE_F64 if name == "float64" else DTYPE_F32


def _out_like(out, shape, dtype, device, noun=None, name="out"):
    """``out`` when it is a contiguous ``dtype`` tensor of ``shape`` on ``device``; a new one for
    None.  ``noun``: how the error text names the dtype (default: as torch prints it); ``name``:
    the argument's name in it."""
    device = _indexed(device)
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if (not isinstance(out, torch.Tensor) or tuple(out.shape) != tuple(shape) or out.dtype != dtype
            or out.device != device or not out.is_contiguous()):
        raise ValueError(f"{name} must be a contiguous {noun or dtype} tensor of shape "
                         f"{tuple(shape)} on {device}")
    return out


def _indexed(device):
    """``device`` as tensors report theirs: a bare "cuda" is torch's current device."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        return torch.device("cuda", torch.cuda.current_device())
    return device


def _extent(t):
    """[first byte, one past the last byte) a kernel addresses through ``t``: from its first to
    its last element, stride gaps included -- ``numel`` elements for a contiguous tensor, ``(3 - 1)
    * stride(0) + field`` for the strided variant views of steric_local_decomp.  None for an empty
    tensor."""
    if t.numel() == 0:
        return None
    last = sum((n - 1) * abs(st) for n, st in zip(t.shape, t.stride()))
    start = t.data_ptr()
    return start, start + (last + 1) * t.element_size()


def _no_overlap(outputs, operands=()):
    """The result-buffer contract: no output of a launch may share a byte with an
    operand or with another output -- the kernels take every pointer ``__restrict__``.
    ``outputs`` / ``operands``: (argument name, tensor or None) pairs of the tensors whose pointers
    go to the launch, that is after any conversion (a converted copy no longer overlaps).  Raises
    ``ValueError`` naming both arguments.  Ranges that only touch do not overlap; an empty tensor
    overlaps nothing; tensors of different devices are different memory.  Host integer
    arithmetic on pointers, shapes and strides: no device query, no synchronisation."""
    outputs = [(n, t, _extent(t)) for n, t in outputs if isinstance(t, torch.Tensor)]
    others = [(n, t, _extent(t)) for n, t in operands if isinstance(t, torch.Tensor)]
    for i, (oname, o, oext) in enumerate(outputs):
        if oext is None:
            continue
        for xname, x, xext in others + outputs[i + 1:]:
            if xext is None or x.device != o.device:
                continue
            if oext[0] < xext[1] and xext[0] < oext[1]:
                raise ValueError(f"{oname} overlaps {xname} in memory: a result buffer must not "
                                 "share bytes with an operand or another result")


def _f64(x, device):
    """Small time-invariant operand -> contiguous float64 device tensor."""
    if isinstance(x, torch.Tensor) and x.is_cuda:
        return x.to(device=device, dtype=torch.float64).contiguous()
    if not isinstance(x, torch.Tensor):
        x = np.asarray(x, dtype=np.float64)
    return hostio.to_device(x, device, torch.float64).contiguous()  # host data: owned staging


def _dtype_code(t, f32_mode):
    if t.dtype == torch.float64:
        return DTYPE_F64
    if t.dtype == torch.float32:
        return F32_MODES[f32_mode]
    raise TypeError(f"thetao/so must be float64 or float32, got {t.dtype}")


def _field(x, nz, ny, nx, name):
    """Validate a streamed field; return (tensor, nt or None, time stride in elements)."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda):
        raise TypeError(f"{name} must be a CUDA/HIP torch tensor")
    if x.dim() == 3:
        if tuple(x.shape) != (nz, ny, nx):
            raise ValueError(f"{name} has shape {tuple(x.shape)}, expected {(nz, ny, nx)}")
        return x.contiguous(), None, 0
    if x.dim() != 4 or tuple(x.shape[1:]) != (nz, ny, nx):
        raise ValueError(f"{name} has shape {tuple(x.shape)}, expected (nt,{nz},{ny},{nx})")
    inner_ok = x.stride(3) == 1 and x.stride(2) == nx and x.stride(1) == ny * nx
    if not inner_ok or x.stride(0) < 0:
        x = x.contiguous()
    return x, x.shape[0], (x.stride(0) if x.shape[0] > 1 else nz * ny * nx)


def _pair(T, S, f32_mode):
    """Common shape logic of the (thetao, so) pair."""
    for name, x in (("thetao", T), ("so", S)):
        if x.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"{name} must be float64 or float32, got {x.dtype}")
    mixed = T.dtype != S.dtype
    if mixed and f32_mode != "faithful":  # "upcast": float64 arithmetic on the stored values
        T, S, mixed = T.double(), S.double(), False
    if (isinstance(T, torch.Tensor) and isinstance(S, torch.Tensor) and T.is_cuda and S.is_cuda
            and T.device != S.device):
        raise ValueError(f"thetao is on {T.device} but so on {S.device}: operands of one call "
                         "must live on one GPU")
    shape3 = tuple(T.shape[-3:])
    nz, ny, nx = shape3
    T, ntT, sT = _field(T, nz, ny, nx, "thetao")
    S, ntS, sS = _field(S, nz, ny, nx, "so")
    if ntT is not None and ntS is not None and ntT != ntS:
        raise ValueError("thetao and so disagree on the number of time steps")
    nt = ntT if ntT is not None else ntS
    squeeze = nt is None
    if squeeze:
        nt = 1
    if nt == 0 or nz * ny * nx == 0:
        raise ValueError(f"empty field: shape {(nt, nz, ny, nx)} has no cells")
    if mixed:
        # numpy evaluates each field's part of the polynomial in that field's precision and joins
        # them in float64 (csrc/eos_device.hpp wright_density_mixed); exact kernels only
        dt = DTYPE_T32_S64 if T.dtype == torch.float32 else DTYPE_T64_S32
    else:
        dt = _dtype_code(T, f32_mode)
    return T, S, nt, nz, ny, nx, sT, sS, dt, squeeze


def _pressure(p, nt, nz, ny, nx, device, allow4d):
    """Classify the pressure operand -> (tensor, p_mode)."""
    if p is None:
        return None, P_SCALAR
    p = _f64(p, device)
    if p.numel() == 1:
        return p.reshape(1), P_SCALAR
    while p.dim() > 3 and p.shape[0] == 1:  # (1,nz,1,1): calc_rho's 4-D broadcast of a z profile
        p = p[0]
    shape = tuple(p.shape)
    if shape in ((nz,), (nz, 1, 1)):  # NB at THIS level a bare (nz,) is a z profile by contract
        return p.reshape(nz), P_ZPROF
    if shape == (nz, ny, nx):
        return p, P_FULL3D
    if allow4d and shape == (nt, nz, ny, nx):
        return p, P_FULL4D
    # anything else that broadcasts against (nz,ny,nx): materialise it (tiny vs the 4-D fields)
    try:
        return p.expand(nz, ny, nx).contiguous(), P_FULL3D
    except RuntimeError:
        pass
    if allow4d:
        return p.expand(nt, nz, ny, nx).contiguous(), P_FULL4D
    raise ValueError(f"pressure of shape {shape} does not broadcast to {(nz, ny, nx)}")


K0_PATHS = {_lib.PATH_GENERIC: "generic", _lib.PATH_FAST: "fast", _lib.PATH_FAST_P3D: "fast_p3d"}
PROMOTE_KINDS = {"d": _lib.KIND_F64, "f": _lib.KIND_F32, "w": _lib.KIND_WEAK}
_PROMOTE_FUNCS = {"inverse_barometer": _lib.FUNC_IBH, "density_ref": _lib.FUNC_DENSITY_REF}


def k0_path(dtype, p_mode, eos, func, plane, sT, sS, flags=0, aligned16=_lib.PATH_ALIGNED_ALL):
    """mlx_path_eos_map: the kernel shape mlx_eos_map (``func`` FUNC_IBH: mlx_inverse_barometer)
    takes for these arguments, all of them the C ABI's codes; ``aligned16`` the PATH_ALIGNED_* bits
    of the operands that are 16-byte aligned.  Returns ("generic" | "fast" | "fast_p3d", the cells
    of a z level one block covers, the time steps one launch takes).  Host arithmetic: no device
    is needed; arguments mlx_eos_map refuses raise ``MomlevelHipError``."""
    import ctypes

    cells, steps = ctypes.c_int64(0), ctypes.c_int64(0)
    rc = _lib.load_path().mlx_path_eos_map(int(dtype), int(p_mode), int(eos), int(func), int(plane),
                                           int(sT), int(sS), int(flags), int(aligned16),
                                           ctypes.byref(cells), ctypes.byref(steps))
    if rc < 0:
        _lib.check(rc, "mlx_path_eos_map")
    return K0_PATHS[rc], int(cells.value), int(steps.value)


def promote_path(kinds, eos="wright", func="density", aligned16=_lib.PATH_ALIGNED_ALL):
    """mlx_path_eos_promote: (the cells a lane takes -- 4, 2 or 1 --, the result dtype) of
    mlx_eos_map_promote for operands of ``kinds``, three letters for T, S and p: d = float64 array,
    f = float32 array, w = python float.  ``aligned16``: the PATH_ALIGNED_* bits of the result and
    of the operands that are 16-byte aligned (a one-element array counts as aligned; the bits of
    python floats and of a pressure the function does not read are ignored).  Host arithmetic: no
    device is needed."""
    import ctypes

    kind = ctypes.c_int(-1)
    fid = _PROMOTE_FUNCS.get(func)
    if fid is None:
        fid = FUNC_IDS[func]
    rc = _lib.load_path().mlx_path_eos_promote(*(PROMOTE_KINDS[k] for k in kinds),
                                               EOS_IDS[eos.lower()], fid, int(aligned16),
                                               ctypes.byref(kind))
    if rc < 0:
        _lib.check(rc, "mlx_path_eos_promote")
    return rc, (torch.float32 if kind.value == _lib.KIND_F32 else torch.float64)


def _is16(t):
    return t is not None and t.data_ptr() % 16 == 0


def _k0_call(T, S, p, eos, f32_mode, flags_of, out):
    """The arguments of one mlx_eos_map / mlx_inverse_barometer call, shared by the launch and by
    eos_map_path: (T, S, dt, pt, p_mode, eos id, nt, nz, plane, sT, sS, flags, out, squeeze)."""
    T, S, nt, nz, ny, nx, sT, sS, dt, squeeze = _pair(T, S, f32_mode)
    pt, p_mode = _pressure(p, nt, nz, ny, nx, T.device, allow4d=True)
    if dt in (DTYPE_T32_S64, DTYPE_T64_S32):
        if out is not None:
            raise ValueError("out= is not available for thetao / so of different dtypes")
        return T, S, dt, pt, p_mode, EOS_IDS[eos.lower()], nt, nz, ny * nx, sT, sS, 0, out, squeeze
    if isinstance(out, torch.Tensor) and squeeze and out.dim() == 3:
        out = out.unsqueeze(0)
    out = _out_like(out, (nt, nz, ny, nx), torch.float64, T.device, "float64")
    _no_overlap([("out", out)], [("thetao", T), ("so", S), ("p", pt)])
    return (T, S, dt, pt, p_mode, EOS_IDS[eos.lower()], nt, nz, ny * nx, sT, sS, flags_of(dt), out,
            squeeze)


def _k0_flags(eos, func, arith):
    if func == "density" and eos.lower() == "wright":
        return lambda dt: _arith_flag(arith, "k0", dt)
    return lambda dt: 0


def eos_map_path(T, S, p, eos="wright", func="density", f32_mode="faithful", arith=None, out=None):
    """The kernel shape ``eos_map`` -- ``func="inverse_barometer"``: ``inverse_barometer`` -- takes
    for these very operands (mlx_path_eos_map on the arguments the call itself would pass): ("generic"
    | "fast" | "fast_p3d", cells of a z level per block, time steps per launch).  Nothing is
    launched.  thetao / so of different dtypes go to eos_map_promote: see promote_path."""
    require_device()
    ibh = func == "inverse_barometer"
    fid = _lib.FUNC_IBH if ibh else FUNC_IDS[func]
    T, S, dt, pt, p_mode, eid, nt, nz, plane, sT, sS, flags, out, _ = _k0_call(
        T, S, p, eos, f32_mode, _k0_flags(eos, func, None if ibh else arith), out)
    if dt in (DTYPE_T32_S64, DTYPE_T64_S32):
        raise ValueError("thetao / so of different dtypes run on eos_map_promote (promote_path)")
    bits = ((_lib.PATH_ALIGNED_T if _is16(T) else 0) | (_lib.PATH_ALIGNED_S if _is16(S) else 0)
            | (_lib.PATH_ALIGNED_OUT if _is16(out) else 0) | (_lib.PATH_ALIGNED_P if _is16(pt) else 0))
    return k0_path(dt, p_mode, eid, fid, plane, sT, sS, flags, bits)


def eos_map(T, S, p, eos="wright", func="density", f32_mode="faithful", arith=None, out=None):
    """K0: pointwise EOS function over a (nt,nz,ny,nx) or (nz,ny,nx) grid -> float64.
    ``arith``: "exact" | "fused" | None = arith_default("k0", dtype) = exact; applies to the Wright
    density only.  ``out``: a contiguous float64 device tensor of the result's shape to write into
    (not for thetao / so of different dtypes); it must not overlap an operand in memory
    (``ValueError``)."""
    require_device()
    T, S, dt, pt, p_mode, eid, nt, nz, plane, sT, sS, flags, out, squeeze = _k0_call(
        T, S, p, eos, f32_mode, _k0_flags(eos, func, arith), out)
    if dt in (DTYPE_T32_S64, DTYPE_T64_S32):
        # thetao and so of different dtypes: numpy's promotion per sub-expression is the promote
        # kernel's job (one cell per thread over the broadcast operands); exact arithmetic only --
        # an explicit arith="fused" is an error here as it is in K1 / K2
        _arith_flag(arith, "k0", dt)
        full = (nt, nz) + tuple(T.shape[-2:])
        ny, nx = full[2:]
        ops = [(x if x.dim() == 4 else x.unsqueeze(0)).expand(full).reshape(-1) for x in (T, S)]
        if pt is not None and pt.numel() > 1:
            pt = {P_ZPROF: lambda q: q.reshape(1, nz, 1, 1), P_FULL3D: lambda q: q.reshape(1, nz, ny, nx),
                  P_FULL4D: lambda q: q}[p_mode](pt).expand(full).reshape(-1)
        res = eos_map_promote(ops[0], ops[1], pt, eos=eos, func=func).reshape(full)
        return res[0] if squeeze else res
    _call(_lib.load(), "mlx_eos_map", T.device, _ptr(T), _ptr(S), dt, _ptr(pt), p_mode,
          eid, FUNC_IDS[func], nt, nz, plane, sT, sS, flags, _ptr(out))
    return out[0] if squeeze else out


def inverse_barometer(T, S, p, gravity=9.8, eos="wright", f32_mode="faithful", out=None):
    """pso * (-1 / (rho(T,S,pso) * gravity)) on a (nt,nz,ny,nx)/(nz,ny,nx) grid -> float64.
    ``out``: a contiguous float64 device tensor of the result's shape to write into; it must not
    overlap an operand in memory (``ValueError``)."""
    require_device()
    T, S, dt, pt, p_mode, eid, nt, nz, plane, sT, sS, _, out, squeeze = _k0_call(
        T, S, p, eos, f32_mode, lambda dt: 0, out)
    if out is None:  # (thetao / so of different dtypes: refused by the library below)
        out = torch.empty((nt, nz) + tuple(T.shape[-2:]), dtype=torch.float64, device=T.device)
    _call(_lib.load(), "mlx_inverse_barometer", T.device, _ptr(T), _ptr(S), dt, _ptr(pt), p_mode,
          eid, float(gravity), nt, nz, plane, sT, sS, _ptr(out))
    return out[0] if squeeze else out


def _promote_call(T, S, p, eos, func):
    """The operands of one mlx_eos_map_promote call, shared by the launch and by
    eos_map_promote_path: (device, n, keep-alive list, the nine operand arguments, func id, kinds,
    the PATH_ALIGNED_* bits of the operands, the (name, tensor) pairs the kernel reads)."""
    import ctypes

    if p is None and (eos.lower() != "linear" or func in ("inverse_barometer", "density_ref")):
        raise TypeError("p must not be None (only the linear EOS ignores the pressure)")
    tensors = [x for x in (T, S, p) if isinstance(x, torch.Tensor)]
    if not tensors:
        raise TypeError("at least one operand must be a device tensor")
    device = tensors[0].device
    n = max(int(x.numel()) for x in tensors)
    keep, read, args, kinds, aligned = [], [], [], "", 0
    bit ={"T": _lib.PATH_ALIGNED_T, "S": _lib.PATH_ALIGNED_S, "p": _lib.PATH_ALIGNED_P}
    for name, x in (("T", T), ("S", S), ("p", p)):
        if x is None:
            if name != "p":
                raise TypeError(f"{name} must not be None")
            args += [None, _lib.KIND_WEAK, 0]
            kinds += "w"
        elif isinstance(x, torch.Tensor):
            if not x.is_cuda or x.device != device:
                raise ValueError("operands of one call must live on one GPU")
            if x.dtype not in (torch.float32, torch.float64):
                raise TypeError(f"{name} must be float32 or float64, not {x.dtype}")
            if x.numel() not in (1, n):
                raise ValueError(f"{name} has {x.numel()} elements, expected 1 or {n}")
            x = x.contiguous()
            keep.append(x)
            read.append((name, x))
            stride = 1 if x.numel() == n and n > 1 else 0
            args += [x.data_ptr(), _lib.KIND_F32 if x.dtype == torch.float32 else _lib.KIND_F64,
                     stride]
            kinds += "f" if x.dtype == torch.float32 else "d"
            if stride == 0 or _is16(x):
                aligned |= bit[name]
        else:
            w = ctypes.c_double(float(x))
            keep.append(w)
            args += [ctypes.addressof(w), _lib.KIND_WEAK, 0]
            kinds += "w"
    fid = _PROMOTE_FUNCS.get(func)
    if fid is None:
        fid = FUNC_IDS[func]
    return device, n, keep, args, fid, kinds, aligned, read


def eos_map_promote_path(T, S, p, eos="wright", func="density", out=None):
    """(cells a lane takes, result dtype) of ``eos_map_promote`` for these very operands
    (mlx_path_eos_promote on the kinds and the alignment the call itself would pass).  Nothing is
    launched."""
    require_device()
    _, _, _, _, _, kinds, aligned, _ = _promote_call(T, S, p, eos, func)
    return promote_path(kinds, eos, func,
                        aligned | (_lib.PATH_ALIGNED_OUT if out is None or _is16(out) else 0))


def eos_map_promote(T, S, p, eos="wright", func="density", gravity=9.8, out=None):
    """K0 under numpy's type promotion (mlx_eos_map_promote; csrc/eos_promote.hpp) for the dtype
    combinations mlx_eos_map does not cover.  Each operand is a python float / int (a WEAK scalar:
    it takes the dtype of the arrays it meets) or a float32 / float64 device tensor of n elements or
    of ONE element (used for every cell); ``p`` may be None for the linear EOS.  ``func`` may also
    be "inverse_barometer" (``gravity`` a python float) or, for the linear EOS, "density_ref" (``p``
    then carries the constant term RHO_T0_S0 - rho_ref of eos/linear.py:55).  Returns a device tensor of n elements in
    numpy's result dtype (float32 when no float64 array takes part) holding numpy's values.
    ``out``: a contiguous 8-byte aligned device tensor of n elements of that dtype (promote_path
    tells it) to write into; it must not overlap an operand in memory (``ValueError``; DESIGN.md
    3.0)."""
    import ctypes

    require_device()
    device, n, keep, args, fid, kinds, _, read = _promote_call(T, S, p, eos, func)
    if out is not None:
        out = _out_like(out, (n,), promote_path(kinds, eos, func)[1], device)
        _no_overlap([("out", out)], read)
    buf = torch.empty(n, dtype=torch.float64, device=device) if out is None else out
    kind = ctypes.c_int(-1)
    _call(_lib.load(), "mlx_eos_map_promote", device, *args, EOS_IDS[eos.lower()], fid,
          float(gravity), n, _ptr(buf), ctypes.byref(kind))
    if out is not None:
        return out
    if kind.value == _lib.KIND_F32:  # the kernel stored n float32 values at the start of the buffer
        return buf.view(torch.float32)[:n]
    return buf


def gradient_coefficients(z):
    """numpy.gradient's per-level coefficients for ``edge_order=2`` along a coordinate ``z`` (what
    xarray's ``differentiate(zcoord, edge_order=2)`` evaluates; derived.py:399-400, :752-753),
    computed on the host from the coordinate with numpy's own expressions, operator for operator.
    Returns (coef (nz,3) float64, uniform, two_dx): level k's derivative is
    ``a*f[k-1] + b*f[k] + c*f[k+1]`` (level 0: on levels 0,1,2; level nz-1: on the last three);
    for evenly spaced levels -- numpy's test: every np.diff equals the first -- the interior is
    ``(f[k+1] - f[k-1]) / two_dx`` instead and only the edge rows of ``coef`` are used."""
    z = np.asarray(z)
    if z.ndim != 1:
        raise ValueError("distances must be either scalars or 1d")
    n = z.shape[0]
    if n < 3:
        raise ValueError("Shape of array too small to calculate a numerical gradient, "
                         "at least (edge_order + 1) elements are required.")
    if np.issubdtype(z.dtype, np.integer):
        z = z.astype(np.float64)
    diffx = np.diff(z)
    coef = np.zeros((n, 3), dtype=np.float64)
    if (diffx == diffx[0]).all():
        dx = diffx[0]
        coef[0] = (-1.5 / dx, 2.0 / dx, -0.5 / dx)
        coef[-1] = (0.5 / dx, -2.0 / dx, 1.5 / dx)
        return coef, True, float(2.0 * dx)
    dx1, dx2 = diffx[0:-1], diffx[1:]
    coef[1:-1, 0] = -(dx2) / (dx1 * (dx1 + dx2))
    coef[1:-1, 1] = (dx2 - dx1) / (dx1 * dx2)
    coef[1:-1, 2] = dx1 / (dx2 * (dx1 + dx2))
    dx1, dx2 = diffx[0], diffx[1]
    coef[0] = (-(2.0 * dx1 + dx2) / (dx1 * (dx1 + dx2)), (dx1 + dx2) / (dx1 * dx2),
               -dx1 / (dx2 * (dx1 + dx2)))
    dx1, dx2 = diffx[-2], diffx[-1]
    coef[-1] = ((dx2) / (dx1 * (dx1 + dx2)), -(dx2 + dx1) / (dx1 * dx2),
                (2.0 * dx2 + dx1) / (dx2 * (dx1 + dx2)))
    return coef, False, 0.0


def stratification(T, S, p, z, func="n2", eos="wright", gravity=-9.8, f32_mode="faithful"):
    """mlx_stratification: N^2 (``func="n2"``, derived.py:328-411) or the stability angle
    (``"turner"``, derived.py:714-766) in one pass over device fields laid out (nt, nz, plane)
    -- z the middle axis, nt / plane the products of the dimensions before / after it.  ``z`` the
    level coordinate (nz,); ``p`` None (linear EOS), one value, (nz,) or a (nt, nz, plane) /
    (nz, plane) float64 device tensor.  Returns (nt, nz, plane) float64."""
    require_device()
    if not (isinstance(T, torch.Tensor) and isinstance(S, torch.Tensor) and T.is_cuda and S.is_cuda):
        raise TypeError("thetao and so must be CUDA/HIP torch tensors")
    if T.dim() != 3 or T.shape != S.shape:
        raise ValueError(f"thetao {tuple(T.shape)} and so {tuple(S.shape)} must both be (nt, nz, plane)")
    if T.dtype != S.dtype:
        raise TypeError("thetao and so of different dtypes: convert one of them")
    dt = _dtype_code(T, f32_mode)
    T, S = T.contiguous(), S.contiguous()
    nt, nz, plane = (int(v) for v in T.shape)
    if nt == 0 or plane == 0:
        raise ValueError(f"empty field: shape {(nt, nz, plane)} has no cells")
    coef, uniform, two_dx = gradient_coefficients(z)
    if coef.shape[0] != nz:
        raise ValueError("when 1d, distances must match the length of the corresponding dimension")
    if eos.lower() == "linear":
        pt, strides = None, (0, 0, 0)
    else:
        if p is None:
            raise TypeError("p must not be None for the Wright EOS")
        pt = _f64(p, T.device)
        shape = tuple(pt.shape)
        if pt.numel() == 1:
            pt, strides = pt.reshape(1), (0, 0, 0)
        elif shape == (nz,):
            strides = (0, 1, 0)
        elif shape == (nz, plane):
            strides = (0, plane, 1)
        elif shape == (nt, nz, plane):
            strides = (nz * plane, plane, 1)
        else:
            raise ValueError(f"pressure of shape {shape} is none of (), ({nz},), ({nz},{plane}), "
                             f"({nt},{nz},{plane})")
    coef_dev = _f64(coef, T.device)
    out = torch.empty((nt, nz, plane), dtype=torch.float64, device=T.device)
    _call(_lib.load(), "mlx_stratification", T.device, _ptr(T), _ptr(S), dt, _ptr(pt), *strides,
          EOS_IDS[eos.lower()], {"n2": _lib.STRAT_N2, "turner": _lib.STRAT_TURNER}[func],
          _ptr(coef_dev), int(uniform), float(two_dx), float(gravity), nt, nz, plane, _ptr(out))
    return out


def adjust_negative_n2(n2, lead0_rows, dz=None, want_adjusted=True):
    """mlx_adjust_negative_n2 on a (nt, nz, plane) float64 device field (see the header for
    ``lead0_rows``).  Returns (adjusted or None, speed or None): ``speed`` (nt, plane), the column
    sum of derived.py:822, when ``dz`` (nz, plane) is given."""
    require_device()
    if n2.dim() != 3:
        raise ValueError("n2 must be (nt, nz, plane)")
    n2 = n2.to(torch.float64).contiguous()
    nt, nz, plane = (int(v) for v in n2.shape)
    adjusted = torch.empty_like(n2) if want_adjusted else None
    speed = dzt = None
    if dz is not None:
        dzt = _f64(dz, n2.device)
        if tuple(dzt.shape) != (nz, plane):
            raise ValueError(f"dz has shape {tuple(dzt.shape)}, expected {(nz, plane)}")
        speed = torch.empty((nt, plane), dtype=torch.float64, device=n2.device)
    _call(_lib.load(), "mlx_adjust_negative_n2", n2.device, _ptr(n2), nt, nz, plane,
          int(lead0_rows), _ptr(dzt), _ptr(adjusted), _ptr(speed))
    return adjusted, speed


def wave_speed_where_time0(n2_t0, speed):
    """mlx_wave_speed_where_time0: (nz, plane) condition field x (nt, plane) speeds ->
    (nz, plane, nt)."""
    require_device()
    nz, plane = (int(v) for v in n2_t0.shape)
    nt = int(speed.shape[0])
    out = torch.empty((nz, plane, nt), dtype=torch.float64, device=speed.device)
    n2_t0, speed = n2_t0.contiguous(), speed.contiguous()
    _call(_lib.load(), "mlx_wave_speed_where_time0", speed.device, _ptr(n2_t0), _ptr(speed), nt, nz,
          plane, _ptr(out))
    return out


def skip_dry_default():
    """Land / sub-bottom skipping is exact, so it is on unless MOMLEVEL_AMD_SKIP_DRY=0."""
    import os

    return os.environ.get("MOMLEVEL_AMD_SKIP_DRY", "1") != "0"


def _launch_flags(skip_dry, arith, t_chunk, kernel, dtype):
    if skip_dry is None:
        skip_dry = skip_dry_default()
    flags = (_lib.FLAG_SKIP_DRY if skip_dry else 0) | _arith_flag(arith, kernel, dtype)
    if t_chunk:
        flags |= _lib.flag_tchunk(t_chunk)
    return flags


def steric_global_masso(T, S, vol0, p, eos="wright", f32_mode="faithful", events=None,
                        skip_dry=None, arith=None, t_chunk=0):
    """K1: masso[t] = sum_{z,y,x} rho(T,S,p) * vol0  (skipna) -> (nt,) float64.

    ``events=(start, end)``: two ``torch.cuda.Event(enable_timing=True)`` recorded on the
    launch stream immediately around the kernel launches (bench.py's per-launch timing).
    ``skip_dry``: MLX_FLAG_SKIP_DRY (None = the default policy, on); results are bit-identical
    either way.  ``arith``: "exact" | "fused" (None = arith_default("k1"): fused).  ``t_chunk``: tuning
    hint, time steps per block (multiple of 8; 0 = library default); never changes a result.
    ``p`` may be time dependent, (nt,nz,ny,nx)-broadcastable (a DataArray ``patm``).
    """
    return _steric_global("mlx_steric_global", T, S, None, vol0, p, eos, f32_mode, events,
                          skip_dry, arith, t_chunk)


def _held_pair(entry, T, S, T0, S0):
    """The reference fields (T0, S0) of an all-variants launch ``entry`` over the validated
    fields T, S: on their device, in their dtypes, contiguous."""
    if T.dim() != 4 or S.dim() != 4:
        raise ValueError(f"{entry[4:]} streams both fields: thetao and so must be 4-D")
    shape3 = tuple(T.shape[1:])
    T0 = T0.to(device=T.device, dtype=T.dtype).contiguous()
    S0 = S0.to(device=T.device, dtype=S.dtype).contiguous()
    if tuple(T0.shape) != shape3 or tuple(S0.shape) != shape3:
        raise ValueError(f"T0 and S0 must be {shape3}")
    return T0, S0


def _steric_global(entry, T, S, held, vol0, p, eos, f32_mode, events, skip_dry, arith, t_chunk):
    """The frame of both K1 entry points (one body, as steric_global_impl on the C side):
    ``held`` None -> mlx_steric_global, (nt,) out; (T0, S0) -> mlx_steric_global_decomp, (4, nt)."""
    require_device()
    T, S, nt, nz, ny, nx, sT, sS, dt, _ = _pair(T, S, f32_mode)
    flags = _launch_flags(skip_dry, arith, t_chunk, "k1", dt)
    dev = T.device
    if held is not None:
        held = _held_pair(entry, T, S, *held)
    vol0 = _f64(vol0, dev)
    if tuple(vol0.shape) != (nz, ny, nx):
        raise ValueError(f"vol0 has shape {tuple(vol0.shape)}, expected {(nz, ny, nx)}")
    pt, p_mode = _pressure(p, nt, nz, ny, nx, dev, allow4d=True)
    lib = _lib.load()
    nbytes = getattr(lib, entry + "_workspace_bytes")(nt, nz, ny * nx)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    out = torch.empty(nt if held is None else (4, nt), dtype=torch.float64, device=dev)
    with _on(dev):
        stream = torch.cuda.current_stream(dev)
        if events is not None:
            events[0].record(stream)
        rc = getattr(lib, entry)(
            _ptr(T), _ptr(S), *map(_ptr, held or ()), dt, _ptr(vol0), _ptr(pt), p_mode,
            EOS_IDS[eos.lower()], nt, nz, ny * nx, sT, sS, flags, _ptr(out), _ptr(ws), nbytes,
            stream.cuda_stream,
        )
        if events is not None:
            events[1].record(stream)
    _lib.check(rc, entry)
    return out


DECOMP_ROWS = ("steric", "thermosteric", "halosteric", "heat")


def steric_global_decomp(T, S, T0, S0, vol0, p, eos="wright", f32_mode="faithful", events=None,
                         skip_dry=None, arith=None, t_chunk=0):
    """K1, all variants in one pass over theta/S: (4, nt) float64, rows DECOMP_ROWS =
    masso of steric / thermosteric (S held at S0) / halosteric (theta held at T0), and
    sum(theta*vol0) (the heat-content integrand; an extension, not in momlevel).  Rows 0-2 are
    bit-identical to three steric_global_masso calls."""
    return _steric_global("mlx_steric_global_decomp", T, S, (T0, S0), vol0, p, eos, f32_mode,
                          events, skip_dry, arith, t_chunk)


def stream_probe(a, b, out=None):
    """Measurement aid: out = a + b with K2's 16-byte nt loads/stores (16 B read + 8 B written per
    element); see mlx_stream_probe.  ``out``: a contiguous float64 device tensor of a's shape that
    overlaps neither stream in memory (``ValueError``)."""
    require_device()
    if _float_code(a, "a") != DTYPE_F64 or _float_code(b, "b") != DTYPE_F64:
        raise TypeError("a and b must be float64")
    if b.numel() != a.numel() or b.device != a.device:
        raise ValueError("a and b must agree in size and device")
    out = _out_like(out, tuple(a.shape), torch.float64, a.device, "float64")
    _no_overlap([("out", out)], [("a", a), ("b", b)])
    _call(_lib.load(), "mlx_stream_probe", a.device, _ptr(a), _ptr(b), a.numel(), _ptr(out))
    return out


def stream_probe_mix(a, b=None, out=None, write=True):
    """Measurement aid: one (``b`` None) or two float32 / float64 streams in, one float64 stream out
    (``write``) or none -- the read:write mix of a held-field / float32 local pass; see
    mlx_stream_probe_mix.  Returns ``out`` (a 1-element tensor, untouched, when ``write`` is False):
    a contiguous float64 device tensor of a's shape (of one element without ``write``) that overlaps
    neither stream in memory (``ValueError``)."""
    require_device()
    dt = _float_code(a, "a")
    if b is not None and (_float_code(b, "b") != dt or b.numel() != a.numel()
                          or b.device != a.device):
        raise ValueError("a and b must agree in dtype, size and device")
    out = _out_like(out, tuple(a.shape) if write else (1,), torch.float64, a.device, "float64")
    _no_overlap([("out", out)], [("a", a), ("b", b)])
    _call(_lib.load(), "mlx_stream_probe_mix", a.device, _ptr(a), _ptr(b), dt, a.numel(), _ptr(out),
          int(bool(write)))
    return out


def valu_probe(iters=4096, device="cuda"):
    """Measurement aid: enqueue the float64 VALU issue-rate probe (mlx_valu_probe) on ``device``'s
    current stream; returns the number of v_fma_f64 lane-instructions the launch issues."""
    require_device()
    device = torch.device(device)
    import ctypes

    out = torch.zeros(1, dtype=torch.float64, device=device)
    n = ctypes.c_int64(0)
    _call(_lib.load(), "mlx_valu_probe", device, int(iters), _ptr(out), ctypes.byref(n))
    return int(n.value)


def fold_mask(rho0, vol0):
    """rho0m = where(vol0 notnull, rho0, NaN) -- prepared once per reference state."""
    require_device()
    rho0 = _f64(rho0, rho0.device)
    vol0 = _f64(vol0, rho0.device)
    out = torch.empty_like(rho0)
    _call(_lib.load(), "mlx_fold_mask", rho0.device, _ptr(rho0), _ptr(vol0), rho0.numel(),
          _ptr(out))
    return out


def _delta_rho_dtype(delta_rho_dtype):
    """``delta_rho_dtype`` of the K2 calls -> torch.float64 | torch.float32"""
    if delta_rho_dtype in (None, torch.float64):
        return torch.float64
    if delta_rho_dtype == torch.float32:
        return torch.float32
    raise ValueError(f"delta_rho_dtype must be torch.float64 or torch.float32, not {delta_rho_dtype!r}")


def _steric_local(entry, T, S, held, rho0m, vol0_surface, p, neg_inv_rhozero, dz, z_i, deptho, eos,
                  f32_mode, skip_dry, arith, delta_rho_dtype=torch.float64):
    """The operands both K2 entry points take (``held``: None, or the (T0, S0) of the all-variants
    launch), validated and on the device -> (device, (nt, nz, ny, nx), launch): ``launch(*outputs)``
    enqueues ``entry`` with the output arguments that follow the common ones.
    ``delta_rho_dtype`` torch.float32: MLX_FLAG_DRHO_F32 -- the delta_rho output (and its variant
    stride) are in float32 elements."""
    require_device()
    T, S, nt, nz, ny, nx, sT, sS, dt, _ = _pair(T, S, f32_mode)
    flags = _launch_flags(skip_dry, arith, 0, "k2", dt)
    if delta_rho_dtype == torch.float32:
        flags |= _lib.FLAG_DRHO_F32
    dev = T.device
    if held is not None:
        held = _held_pair(entry, T, S, *held)
    rho0m = _f64(rho0m, dev)
    vol0_surface = _f64(vol0_surface, dev)
    if tuple(rho0m.shape) != (nz, ny, nx) or tuple(vol0_surface.shape) != (ny, nx):
        raise ValueError("rho0m must be (nz,ny,nx) and vol0_surface (ny,nx)")
    pt, p_mode = _pressure(p, nt, nz, ny, nx, dev, allow4d=True)
    if dz is not None:
        dz = _f64(dz, dev)
        if tuple(dz.shape) != (nz, ny, nx):
            raise ValueError("dz must be (nz,ny,nx)")
    else:
        z_i = _f64(z_i, dev)
        deptho = _f64(deptho, dev)
        if z_i.numel() != nz + 1 or tuple(deptho.shape) != (ny, nx):
            raise ValueError("z_i must have nz+1 entries and deptho be (ny,nx)")

    def launch(*outputs):
        _call(_lib.load(), entry, dev, _ptr(T), _ptr(S), *map(_ptr, held or ()), dt, _ptr(rho0m),
              _ptr(vol0_surface), _ptr(dz), _ptr(z_i), _ptr(deptho), _ptr(pt), p_mode,
              EOS_IDS[eos.lower()], float(neg_inv_rhozero), nt, nz, ny * nx, sT, sS, flags,
              *outputs)

    read = [("thetao", T), ("so", S)] + list(zip(("T0", "S0"), held or ())) + [
        ("rho0m", rho0m), ("vol0_surface", vol0_surface), ("dz", dz), ("z_i", z_i),
        ("deptho", deptho), ("p", pt)]
    return dev, (nt, nz, ny, nx), launch, read


def steric_local(T, S, rho0m, vol0_surface, p, neg_inv_rhozero, dz=None, z_i=None,
                 deptho=None, eos="wright", f32_mode="faithful", want_delta_rho=True,
                 delta_rho_out=None, eta_out=None, skip_dry=None, arith=None,
                 delta_rho_dtype=torch.float64):
    """K2: (delta_rho (nt,nz,ny,nx) or None, eta (nt,ny,nx)).  ``skip_dry``, ``arith``: see
    steric_global_masso.  ``p`` may be time dependent (4-D).
    ``delta_rho_dtype`` torch.float32 (an extension; the default is float64): the kernel rounds each
    delta_rho value to float32 right before storing it -- ``float32(float64 delta_rho)`` bit for
    bit, half the bytes -- while eta is summed from the unrounded terms and stays float64, the
    same bits as without it.  A ``delta_rho_out`` must be of that dtype.
    ``delta_rho_out`` (nt,nz,ny,nx) / ``eta_out`` (nt,ny,nx) float64: contiguous device tensors of
    exactly these shapes that overlap neither an operand nor each other in memory (``ValueError``;
    DESIGN.md 3.0)."""
    ddt = _delta_rho_dtype(delta_rho_dtype)
    dev, (nt, nz, ny, nx), launch, read = _steric_local(
        "mlx_steric_local", T, S, None, rho0m, vol0_surface, p, neg_inv_rhozero, dz, z_i, deptho,
        eos, f32_mode, skip_dry, arith, ddt if want_delta_rho else torch.float64)
    drho = None
    if want_delta_rho:
        # (never a silent reinterpretation of the buffer's elements: delta_rho_dtype decides)
        drho = _out_like(delta_rho_out, (nt, nz, ny, nx), ddt, dev, name="delta_rho_out")
    eta = _out_like(eta_out, (nt, ny, nx), torch.float64, dev, "float64", name="eta_out")
    _no_overlap([("delta_rho_out", drho), ("eta_out", eta)], read)
    launch(_ptr(drho), _ptr(eta))
    return drho, eta


LOCAL_DECOMP_ROWS = ("steric", "thermosteric", "halosteric")


def steric_local_decomp(T, S, T0, S0, rho0m, vol0_surface, p, neg_inv_rhozero, dz=None, z_i=None,
                        deptho=None, eos="wright", f32_mode="faithful", want_delta_rho=True,
                        delta_rho_out=None, eta_out=None, skip_dry=None, arith=None,
                        delta_rho_dtype=torch.float64):
    """K2, all variants in one pass over theta/S: (delta_rho (3,nt,nz,ny,nx) or None,
    eta (3,nt,ny,nx)), variant order LOCAL_DECOMP_ROWS; each field bit-identical to its
    steric_local call.  ``delta_rho_out`` / ``eta_out``: optional (3, nt, ...) float64 device
    tensors (or views whose variant axis has any stride, e.g. ``full[:, t0:t1]``).
    ``delta_rho_dtype``: as in steric_local (``delta_rho_out`` then float32; eta stays float64).
    Neither output may overlap an operand or the other output in memory, over the whole extent from
    its first variant to its last, stride gaps included (``ValueError``)."""
    ddt = _delta_rho_dtype(delta_rho_dtype)
    dev, (nt, nz, ny, nx), launch, read = _steric_local(
        "mlx_steric_local_decomp", T, S, (T0, S0), rho0m, vol0_surface, p, neg_inv_rhozero, dz, z_i,
        deptho, eos, f32_mode, skip_dry, arith, ddt if want_delta_rho else torch.float64)

    def variant_major(x, shape, dtype=torch.float64):
        """(3, nt, ...) device tensor of ``dtype`` whose per-variant fields are contiguous"""
        if (not isinstance(x, torch.Tensor) or tuple(x.shape) != shape or x.dtype != dtype
                or x.device != dev):
            raise ValueError(f"output must be a {dtype} {shape} tensor on {dev}")
        if not x[0].is_contiguous() or x.stride(0) < x[0].numel():
            raise ValueError("each variant's field must be contiguous")
        return x

    drho = None
    if want_delta_rho:
        drho = delta_rho_out if delta_rho_out is not None else torch.empty(
            (3, nt, nz, ny, nx), dtype=ddt, device=dev)
        variant_major(drho, (3, nt, nz, ny, nx), ddt)
    eta = eta_out if eta_out is not None else torch.empty((3, nt, ny, nx), dtype=torch.float64,
                                                           device=dev)
    variant_major(eta, (3, nt, ny, nx))
    _no_overlap([("delta_rho_out", drho), ("eta_out", eta)], read)
    launch(_ptr(drho), drho.stride(0) if drho is not None else 0, _ptr(eta), eta.stride(0))
    return drho, eta


def nansum(x):
    """skipna sum of a float64 device tensor -> 0-d device tensor."""
    require_device()
    x = _f64(x, x.device).reshape(-1)
    lib = _lib.load()
    nbytes = lib.mlx_nansum_workspace_bytes(x.numel())
    ws = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=x.device)
    out = torch.empty(1, dtype=torch.float64, device=x.device)
    _call(lib, "mlx_nansum", x.device, _ptr(x), x.numel(), _ptr(out), _ptr(ws), nbytes)
    return out[0]


def masso(rho, vol):
    """Standalone calc_masso: rho (nt, n3), vol (n3,) or (nt, n3) -> sum(rho*vol) [skipna], (nt,)."""
    require_device()
    rho = _f64(rho, rho.device)
    vol = _f64(vol, rho.device)
    if rho.dim() != 2:
        raise ValueError("rho must be (nt, n3)")
    nt, n3 = rho.shape
    if tuple(vol.shape) == (n3,):
        vstride = 0
    elif tuple(vol.shape) == (nt, n3):
        vstride = n3
    else:
        raise ValueError("vol must be (n3,) or (nt, n3)")
    lib = _lib.load()
    out = torch.empty(nt, dtype=torch.float64, device=rho.device)
    step = 32768  # the kernel's grid.y carries the time axis (<= 65535)
    nbytes = lib.mlx_steric_global_workspace_bytes(min(nt, step), 1, n3)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=rho.device)
    for t0 in range(0, nt, step):
        t1 = min(t0 + step, nt)
        _call(lib, "mlx_masso", rho.device, _ptr(rho[t0:t1]), _ptr(vol[t0:t1] if vstride else vol),
              t1 - t0, n3, vstride, _ptr(out[t0:t1]), _ptr(ws), nbytes)
    return out


def group_weighted_mean(x, w, group_len, out=None):
    """Per-group weighted mean over the leading axis (annual_average's arithmetic): x (nt, ...)
    with nt = ngroups*group_len, w (nt,) -> (ngroups, ...); NaNs carry no weight.  ``out``: a
    contiguous float64 device tensor of that shape that overlaps neither x nor w in memory
    (``ValueError``)."""
    require_device()
    x = _f64(x, x.device)
    w = _f64(w, x.device).reshape(-1)
    nt = x.shape[0]
    if nt % group_len or w.numel() != nt:
        raise ValueError("the time axis must hold whole groups and one weight per step")
    ngroups = nt // group_len
    n = x[0].numel()
    out = _out_like(out, (ngroups,) + tuple(x.shape[1:]), torch.float64, x.device, "float64")
    _no_overlap([("out", out)], [("x", x), ("w", w)])
    _call(_lib.load(), "mlx_group_weighted_mean", x.device, _ptr(x), _ptr(w), ngroups, group_len, n,
          _ptr(out))
    return out


# ---------------------------------------------------------------------------------------
# the trend kernels (include/momlevel_trend.h; csrc/momlevel_trend.hip)
# ---------------------------------------------------------------------------------------
APPLY_MODES = {
    "remove": _lib.APPLY_REMOVE, "correct": _lib.APPLY_CORRECT, "trend": _lib.APPLY_TREND,
    "trend_anom": _lib.APPLY_TREND_ANOM, "model_resid": _lib.APPLY_MODEL_RESID,
    "model": _lib.APPLY_MODEL,
}


def _time_record(y):
    """A (time, ...) device record as the kernels read it: C-contiguous, float32 kept (widened in
    registers), anything else float64.  Returns (tensor, nt, cells, dtype code)."""
    if not (isinstance(y, torch.Tensor) and y.is_cuda):
        raise TypeError("the record must be a device tensor")
    if y.dim() < 1 or y.shape[0] < 1:
        raise ValueError("the record needs a leading time axis")
    if y.dtype not in (torch.float32, torch.float64):
        y = y.to(torch.float64)
    y = y.contiguous()
    return y, y.shape[0], y[0].numel(), _float_code(y, "the record")


def _fit_workspace(lib, nt, n, nterms, device):
    nbytes = lib.mlx_time_fit_workspace_bytes(nt, n, nterms)
    if n > 0 and nbytes == 0:
        raise ValueError(f"a record of {nt} steps x {n} cells is outside the fit kernels' range")
    return torch.empty(max(nbytes // 8, 2), dtype=torch.float64, device=device), nbytes


def time_linfit(y, xt, s, xmean):
    """NaN-skipping straight-line fit per cell along the leading axis (mlx_time_linfit): y (nt, ...)
    float32 / float64, xt (nt,) = (x - xmean) / s  ->  (slope, intercept), float64, shaped
    y.shape[1:].  Cells with fewer than 2 valid steps give NaN."""
    require_device()
    lib = _lib.load_trend()
    y, nt, n, code = _time_record(y)
    xt = _f64(xt, y.device).reshape(-1)
    if xt.numel() != nt:
        raise ValueError("one xt per time step")
    slope = torch.empty(y.shape[1:], dtype=torch.float64, device=y.device)
    intercept = torch.empty_like(slope)
    if n == 0:
        return slope, intercept
    ws, nbytes = _fit_workspace(lib, nt, n, 5, y.device)
    _call(lib, "mlx_time_linfit", y.device, _ptr(y), code, _ptr(xt), nt, n, float(s), float(xmean),
          _ptr(slope), _ptr(intercept), _ptr(ws), nbytes)
    return slope, intercept


def time_project(y, P):
    """coef[k] = sum_t P[t, k] * y[t] per cell (mlx_time_project): y (nt, ...), P (nt, K) with
    K <= 8  ->  (K, ...) float64.  NaN propagates: one NaN step makes the cell's K values NaN."""
    require_device()
    lib = _lib.load_trend()
    y, nt, n, code = _time_record(y)
    P = _f64(P, y.device)
    if P.dim() != 2 or P.shape[0] != nt or not 1 <= P.shape[1] <= _lib.TREND_MAX_TERMS:
        raise ValueError(f"P must be (nt, K) with 1 <= K <= {_lib.TREND_MAX_TERMS}")
    K = P.shape[1]
    coef = torch.empty((K,) + tuple(y.shape[1:]), dtype=torch.float64, device=y.device)
    if n == 0:
        return coef
    ws, nbytes = _fit_workspace(lib, nt, n, K, y.device)
    _call(lib, "mlx_time_project", y.device, _ptr(y), code, _ptr(P), K, nt, n, _ptr(coef), _ptr(ws),
          nbytes)
    return coef


def time_apply(y, mode, xm, a, b=None, out=None):
    """The elementwise pass (mlx_time_apply).  Straight-line modes "remove" / "correct" /
    "trend" / "trend_anom": xm = x (nt,), a = slope, b = intercept ("remove").  Model modes
    "model_resid" / "model": xm = M (K, nt), a = coef (K, ...).  ``y`` (nt, ...) may be None in the
    modes that do not read it.  Returns (nt, ...) float64 (``out`` when given: a contiguous
    float64 device tensor of that shape that overlaps no operand in memory; ``ValueError``
    otherwise)."""
    require_device()
    lib = _lib.load_trend()
    code_mode = APPLY_MODES[mode]
    model = mode in ("model_resid", "model")
    reads_y = mode in ("remove", "correct", "model_resid")
    a = _f64(a, a.device)
    device = a.device
    xm = _f64(xm, device)
    if model and (xm.dim() != 2 or a.dim() < 1 or a.shape[0] != xm.shape[0]):
        raise ValueError("model modes take M (K, nt) and coef (K, ...)")
    K = xm.shape[0] if model else 0
    nt = xm.shape[1] if model else xm.numel()
    cells_shape = tuple(a.shape[1:]) if model else tuple(a.shape)
    n = int(np.prod(cells_shape, dtype=np.int64))
    code = DTYPE_F64
    if reads_y:
        y, ynt, yn, code = _time_record(y)
        if ynt != nt or tuple(y.shape[1:]) != cells_shape:
            raise ValueError("y must be (nt,) + the cells' shape")
    else:
        y = None
    if mode == "remove":
        if b is None:
            raise ValueError('mode "remove" needs the intercept')
        b = _f64(b, device)
        if tuple(b.shape) != cells_shape:
            raise ValueError("slope and intercept must agree in shape")
    else:
        b = None
    out = _out_like(out, (nt,) + cells_shape, torch.float64, device, "float64")
    _no_overlap([("out", out)], [("y", y), ("xm", xm), ("a", a), ("b", b)])
    if n == 0:
        return out
    step = 65535 * 64  # the kernel's grid.y carries the time axis in windows of 64 steps
    for t0 in range(0, nt, step):
        t1 = min(t0 + step, nt)
        if model:
            xs = xm[:, t0:t1].contiguous() if (t0, t1) != (0, nt) else xm
        else:
            xs = xm[t0:t1]
            if mode == "trend_anom" and t0:
                raise ValueError("trend_anom: time axis too long for one call")
        _call(lib, "mlx_time_apply", device, _ptr(y[t0:t1]) if reads_y else None, code, code_mode,
              _ptr(xs), _ptr(a), _ptr(b), K, t1 - t0, n, _ptr(out[t0:t1]))
    return out


# ---------------------------------------------------------------------------------------
# the grouped time statistic (include/momlevel_clim.h; csrc/momlevel_clim.hip)
# ---------------------------------------------------------------------------------------
STAT_IDS = {"mean": _lib.STAT_MEAN, "std": _lib.STAT_STD, "min": _lib.STAT_MIN,
            "max": _lib.STAT_MAX}


def check_groups(steps, offsets, nt):
    """The host-side mirror of a group list as the kernel reads it: ``(steps int32 (nsel),
    offsets int64 (ngroups + 1))``, or ``ValueError`` -- a step outside [0, nt), offsets that
    decrease or leave [0, nsel], no group or no step at all.  Touches no device."""
    steps = np.ascontiguousarray(np.asarray(steps).reshape(-1))
    offsets = np.ascontiguousarray(np.asarray(offsets).reshape(-1))
    if steps.dtype.kind not in "iu" or offsets.dtype.kind not in "iu":
        raise ValueError("steps and offsets must hold integers")
    if steps.size < 1 or offsets.size < 2:
        raise ValueError("need at least one step and one group (offsets holds ngroups + 1 values)")
    if int(steps.min()) < 0 or int(steps.max()) >= int(nt):
        raise ValueError(f"steps must lie in [0, {int(nt)})")
    if int(offsets[0]) < 0 or int(offsets[-1]) > steps.size or np.any(np.diff(offsets.astype(np.int64)) < 0):
        raise ValueError(f"offsets must not decrease and must lie in [0, {steps.size}]")
    return steps.astype(np.int32), offsets.astype(np.int64)


class DeviceGroups:
    """A checked group list on the device: what ``time_group_stat`` takes in place of host
    ``steps`` / ``offsets`` when the same groups serve several calls."""

    def __init__(self, steps, offsets, nt, device):
        steps, offsets = check_groups(steps, offsets, nt)
        self.nt, self.nsel, self.ngroups = int(nt), int(steps.size), int(offsets.size - 1)
        # (integer lists: a plain copy -- hostio's staging carries floating fields only)
        self.steps = torch.from_numpy(steps).to(device)
        self.offsets = torch.from_numpy(offsets).to(device)


def upload_groups(steps, offsets, nt, device):
    """``check_groups``, then the two lists on ``device`` (a ``DeviceGroups``)."""
    return DeviceGroups(steps, offsets, nt, torch.device(device))


def time_group_stat(y, steps, offsets=None, stat="mean", out=None):
    """NaN-skipping ``stat`` ("mean", "std", "min", "max") over groups of steps of the leading
    axis (mlx_clim_group_stat): y (nt, ...) float32 / float64 on the device; group g is
    ``steps[offsets[g]:offsets[g + 1]]``, visited in that order  ->  (ngroups, ...) of y's dtype.
    ``steps`` / ``offsets`` are host integer sequences, checked here before they are uploaded, or
    ``steps`` is a ``DeviceGroups`` made by ``upload_groups`` (``offsets`` None).  float64 results
    are bit-identical to numpy's nanmean / nanstd / nanmin / nanmax over axis 0 of ``y[sel]``;
    float32 records are accumulated in float64 and rounded once.  ``out``: a contiguous device
    tensor of the result's shape and dtype that overlaps no operand in memory (``ValueError``;
    DESIGN.md 3.0)."""
    require_device()
    lib = _lib.load_clim()
    if stat not in STAT_IDS:
        raise ValueError(f"stat must be one of {sorted(STAT_IDS)}, got '{stat}'")
    y, nt, n, code = _time_record(y)
    if isinstance(steps, DeviceGroups):
        groups = steps
        if offsets is not None:
            raise ValueError("a DeviceGroups carries its own offsets")
        if groups.nt != nt or groups.steps.device != y.device:
            raise ValueError("the groups were made for another record length or device")
    else:
        groups = DeviceGroups(steps, offsets, nt, y.device)
    shape = (groups.ngroups,) + tuple(y.shape[1:])
    out = _out_like(out, shape, y.dtype, y.device)
    _no_overlap([("out", out)], [("y", y), ("steps", groups.steps), ("offsets", groups.offsets)])
    if n == 0:
        return out
    _call(lib, "mlx_clim_group_stat", y.device, _ptr(y), code, _ptr(groups.steps),
          _ptr(groups.offsets), groups.nsel, groups.ngroups, nt, n, STAT_IDS[stat], _ptr(out))
    return out


# ---------------------------------------------------------------------------------------
# tide gauges (include/momlevel_gauge.h; csrc/momlevel_gauge.hip)
# ---------------------------------------------------------------------------------------
def _gauge_operand(x, device, what):
    """lat / lon / mask as the prepare kernel reads them: flat, contiguous, on ``device``; float32
    stays (widened exactly in registers), every other dtype becomes float64."""
    if isinstance(x, torch.Tensor):
        if x.dtype not in (torch.float32, torch.float64):
            x = x.to(torch.float64)
        return x.to(device).reshape(-1).contiguous()
    x = np.asarray(x)
    if x.dtype.kind not in "fiub":
        raise TypeError(f"{what} must be numeric, got {x.dtype}")
    dt = torch.float32 if x.dtype == np.float32 else torch.float64
    x = np.ascontiguousarray(x.reshape(-1), dtype=np.float32 if dt == torch.float32 else np.float64)
    return hostio.to_device(x, device, dt).contiguous()


def gauge_prepare(lat, lon, mask=None, device=None):
    """Unit vectors, radians and validity of ``n`` positions (mlx_gauge_prepare): lat, lon in
    degrees, of any shape with ``n`` elements, numpy or device tensors; ``mask`` optional, same
    element count -- a point is valid iff its mask value == 1.0 exactly (NaN, 0.5: dry) and its
    coordinates are finite  ->  ``(table (5, n) float64, valid (n) uint8)`` on the device: rows x,
    y, z (+inf for an invalid point), phi, lam (NaN for one).  Gauges are prepared the same way."""
    require_device()
    lib = _lib.load_gauge()
    if device is None:
        device = next((x.device for x in (lat, lon, mask)
                       if isinstance(x, torch.Tensor) and x.is_cuda), torch.device("cuda"))
    device = torch.device(device)
    lat = _gauge_operand(lat, device, "lat")
    lon = _gauge_operand(lon, device, "lon")
    if lat.numel() != lon.numel():
        raise ValueError("lat and lon must hold the same number of points")
    if lat.dtype != lon.dtype:
        lat, lon = lat.to(torch.float64), lon.to(torch.float64)
    n = lat.numel()
    mcode = DTYPE_F64
    if mask is not None:
        mask = _gauge_operand(mask, device, "mask")
        if mask.numel() != n:
            raise ValueError("one mask value per point")
        mcode = _float_code(mask, "mask")
    table = torch.empty((_lib.GAUGE_ROWS, n), dtype=torch.float64, device=device)
    valid = torch.empty((n,), dtype=torch.uint8, device=device)
    if n == 0:
        return table, valid
    _call(lib, "mlx_gauge_prepare", device, _ptr(lat), _ptr(lon), _float_code(lat, "lat"),
          _ptr(mask), mcode, n, _ptr(table), _ptr(valid))
    return table, valid


def _gauge_table(t, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.dim() == 2
            and t.shape[0] == _lib.GAUGE_ROWS and t.is_contiguous()):
        raise ValueError(f"{what} must be a contiguous (5, n) float64 device table of gauge_prepare")
    return t


def gauge_nearest(points, gauges, split=0):
    """For every gauge the valid point with the smallest squared chord, ties to the lowest flat
    index (mlx_gauge_nearest): ``points`` (5, n) and ``gauges`` (5, ng) are tables of
    ``gauge_prepare``  ->  ``(index (ng) int64, angle (ng) float64)``: the flat index of the
    winner (-1 when no point is valid) and the haversine angle to it in radians (NaN then).
    ``split``: into how many parts the points are cut over blocks (0: the library's choice); index
    and angle are bit-identical for every value."""
    require_device()
    lib = _lib.load_gauge()
    points, gauges = _gauge_table(points, "points"), _gauge_table(gauges, "gauges")
    if gauges.device != points.device:
        raise ValueError("points and gauges must live on one device")
    split = int(split)
    if split < 0:
        raise ValueError("split must be >= 0")
    n, ng, device = points.shape[1], gauges.shape[1], points.device
    index = torch.full((ng,), -1, dtype=torch.int64, device=device)
    angle = torch.full((ng,), float("nan"), dtype=torch.float64, device=device)
    if n == 0 or ng == 0:
        return index, angle
    nbytes = lib.mlx_gauge_nearest_workspace_bytes(n, ng, split)
    if nbytes == 0:
        raise ValueError(f"{n} points x {ng} gauges is outside the search kernel's range")
    ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=device)
    _call(lib, "mlx_gauge_nearest", device, _ptr(points), n, _ptr(gauges), ng, split, _ptr(index),
          _ptr(angle), _ptr(ws), nbytes)
    return index, angle


def gauge_gather(y, index, out=None):
    """``out[g, r] = y[r, index[g]]`` (mlx_gauge_gather): y (nrest, n) float32 / float64 on the
    device, ``index`` (ng) integers (host sequence or device tensor)  ->  (ng, nrest) of y's dtype,
    each gauge's series contiguous, bits copied.  An index outside [0, n) gives a NaN series.
    ``out``: a contiguous device tensor of that shape and dtype that overlaps neither y nor a
    device ``index`` in memory (``ValueError``)."""
    require_device()
    lib = _lib.load_gauge()
    if isinstance(y, torch.Tensor) and y.is_cuda:
        if y.dim() != 2:
            raise ValueError("the record must be (nrest, n)")
        y = y.contiguous()  # (a strided record is copied, not refused)
    code = _float_code(y, "the record")
    if isinstance(index, torch.Tensor):
        if index.dtype not in (torch.int64, torch.int32, torch.int16, torch.uint8, torch.int8):
            raise TypeError("index must hold integers")
        index = index.to(device=y.device, dtype=torch.int64).reshape(-1).contiguous()
    else:
        host = np.asarray(index).reshape(-1)
        if host.dtype.kind not in "iu":
            raise TypeError("index must hold integers")
        index = torch.from_numpy(np.ascontiguousarray(host, dtype=np.int64)).to(y.device)
    nrest, n = y.shape
    ng = index.numel()
    shape = (ng, nrest)
    out = _out_like(out, shape, y.dtype, y.device)
    _no_overlap([("out", out)], [("y", y), ("index", index)])
    if ng == 0 or nrest == 0:
        return out
    if n == 0:
        return out.fill_(float("nan"))
    _call(lib, "mlx_gauge_gather", y.device, _ptr(y), code, _ptr(index), nrest, n, ng, _ptr(out))
    return out


def spice_map(theta, so, out=None):
    """Flament (2002) spiciness of every cell (mlx_spice_map): ``theta`` and ``so`` contiguous 1-D
    device tensors of equal length, each float32 or float64 on its own  ->  a float64 device tensor
    of that length (``out`` when given; it must not overlap an operand in memory: ``ValueError``,
    DESIGN.md 3.0).  float32 values are widened exactly; all arithmetic is float64."""
    require_device()
    lib = _lib.load_spice()
    tdt, sdt = _float_code(theta, "theta", 1), _float_code(so, "so", 1)
    if so.numel() != theta.numel() or so.device != theta.device:
        raise ValueError("theta and so must agree in length and device")
    n = theta.numel()
    out = _out_like(out, (n,), torch.float64, theta.device, "float64")
    _no_overlap([("out", out)], [("theta", theta), ("so", so)])
    _call(lib, "mlx_spice_map", theta.device, _ptr(theta), tdt, _ptr(so), sdt, n, _ptr(out))
    return out


def vort_tile():
    """(W64, W32, H, bands) of the packed path of the vorticity kernels (include/momlevel_vort.h):
    a wave's tile is W64 float64 / W32 float32 cells wide and H rows high, a block stacks ``bands``
    of them in y."""
    lib = _lib.load_vort()
    return (int(lib.mlx_vort_tile_width(DTYPE_F64)), int(lib.mlx_vort_tile_width(DTYPE_F32)),
            _lib.VORT_TILE_H, _lib.VORT_TILE_BANDS)


def vort_records_per_launch(ny, nx, dtype=torch.float64):
    """Records one launch of the packed path of rel_vort / potential_vorticity takes for a corner
    plane of (ny, nx) and arithmetic in ``dtype`` (mlx_vort_records_per_launch); a call over more is
    cut into launches of that many.  0 where the shape sends the plane cell by cell."""
    return int(_lib.load_vort().mlx_vort_records_per_launch(int(ny), int(nx), _query_dtype(dtype)))


def rel_vort(u, v, dx, dy, area, symmetric=False, out=None):
    """Relative vorticity on the C grid (mlx_vort_rel_vort): ``( -diff_y(u dx) + diff_x(v dy) ) /
    area`` with zero padding.  ``area`` is the (ny, nx) corner plane; with s = int(symmetric) ``u``
    is (nrec, ny - s, nx) and ``v`` (nrec, ny, nx - s), both of ONE dtype; ``dx`` / ``dy`` are their
    2-D metrics, of one dtype with ``area``.  All contiguous device tensors, float32 or float64.
    Returns (nrec, ny, nx): float32 when fields and metrics are all float32, float64 otherwise --
    bit for bit what numpy gives operator for operator.  ``out``: a contiguous device tensor of
    that shape and dtype that overlaps no operand in memory -- the stencil reads its neighbours'
    cells (``ValueError``)."""
    require_device()
    lib = _lib.load_vort()
    fdt = _float_code(u, "u", 3)
    if _float_code(v, "v", 3) != fdt:
        raise TypeError(f"u and v must have the same dtype, got {u.dtype} and {v.dtype}")
    mdt = _float_code(area, "area", 2)
    for name, m in (("dx", dx), ("dy", dy)):
        if _float_code(m, name, 2) != mdt:
            raise TypeError(f"dx, dy and area must have the same dtype, got {m.dtype} for {name} "
                            f"and {area.dtype} for area")
    s = int(bool(symmetric))
    ny, nx = (int(n) for n in area.shape)
    nrec = int(u.shape[0])
    if ny < 1 + s or nx < 1 + s:
        raise ValueError(f"area {tuple(area.shape)}: the corner plane needs at least {1 + s} points "
                         "a side")
    want = {"u": (nrec, ny - s, nx), "v": (nrec, ny, nx - s), "dx": (ny - s, nx), "dy": (ny, nx - s)}
    for name, x in (("u", u), ("v", v), ("dx", dx), ("dy", dy)):
        if tuple(x.shape) != want[name]:
            raise ValueError(f"{name} has shape {tuple(x.shape)}, expected {want[name]} for a corner "
                             f"plane of {(ny, nx)} with symmetric={bool(symmetric)}")
    if any(x.device != u.device for x in (v, dx, dy, area)):
        raise ValueError("u, v, dx, dy and area must live on one device")
    odt = torch.float32 if fdt == DTYPE_F32 and mdt == DTYPE_F32 else torch.float64
    out = _out_like(out, (nrec, ny, nx), odt, u.device)
    _no_overlap([("out", out)], [("u", u), ("v", v), ("dx", dx), ("dy", dy), ("area", area)])
    _call(lib, "mlx_vort_rel_vort", u.device, _ptr(u), _ptr(v), fdt, _ptr(dx), _ptr(dy), _ptr(area),
          mdt, nrec, ny, nx, s, _ptr(out))
    return out


VORT_UNITS = {"m": _lib.VORT_UNITS_M, "cm": _lib.VORT_UNITS_CM}


def potential_vorticity(zeta, coriolis, n2, gravity=9.8, interp=True, symmetric=False, units="m",
                        out=None):
    """Potential vorticity (mlx_vort_pv): ``(zeta + coriolis) * (n2c / gravity)`` and, for
    ``units="cm"``, ``abs((pv / 100) * 1e14)``.  ``zeta`` (nrec, ny, nx) and ``coriolis`` (ny, nx)
    live on the corner plane; ``n2`` is (nrec, ny, nx) without ``interp`` and (nrec, ny - s, nx - s)
    with it (s = int(symmetric)): then n2c is N^2 averaged along x and then along y with zero
    padding, inside the pass.  Each operand float32 or float64 on its own; the result has numpy's
    promotion of the three, and numpy's bits.  ``out``: a contiguous device tensor of the result's
    shape and dtype that overlaps no operand in memory (``ValueError``)."""
    if units not in VORT_UNITS:
        raise ValueError(f"unknown units option `{units}`")
    require_device()
    lib = _lib.load_vort()
    zdt, cdt, ndt = (_float_code(zeta, "zeta", 3), _float_code(coriolis, "coriolis", 2),
                     _float_code(n2, "n2", 3))
    interp = int(bool(interp))
    s = int(bool(symmetric)) if interp else 0
    nrec, ny, nx = (int(n) for n in zeta.shape)
    if tuple(coriolis.shape) != (ny, nx):
        raise ValueError(f"coriolis has shape {tuple(coriolis.shape)}, expected {(ny, nx)}")
    if ny < 1 + s or nx < 1 + s:
        raise ValueError(f"zeta {tuple(zeta.shape)}: the corner plane needs at least {1 + s} points "
                         "a side")
    if tuple(n2.shape) != (nrec, ny - s, nx - s):
        raise ValueError(f"n2 has shape {tuple(n2.shape)}, expected {(nrec, ny - s, nx - s)} for "
                         f"zeta {tuple(zeta.shape)} with interp={bool(interp)}, "
                         f"symmetric={bool(symmetric)}")
    if coriolis.device != zeta.device or n2.device != zeta.device:
        raise ValueError("zeta, coriolis and n2 must live on one device")
    odt = torch.float32 if (zdt, cdt, ndt) == (DTYPE_F32,) * 3 else torch.float64
    out = _out_like(out, (nrec, ny, nx), odt, zeta.device)
    _no_overlap([("out", out)], [("zeta", zeta), ("coriolis", coriolis), ("n2", n2)])
    _call(lib, "mlx_vort_pv", zeta.device, _ptr(zeta), zdt, _ptr(coriolis), cdt, _ptr(n2), ndt,
          nrec, ny, nx, interp, s, float(gravity), VORT_UNITS[units], _ptr(out))
    return out


def rossby_radius(c, f, out=None):
    """``c / abs(f)`` (mlx_vort_rossby): ``c`` a contiguous (outer, plane, inner) device tensor, ``f``
    a contiguous tensor of ``plane`` elements, each float32 or float64; IEEE division, so that
    ``f == 0`` gives the +-inf / NaN numpy gives.  ``out``: a contiguous device tensor of c's shape
    (float32 when both are float32, else float64) that overlaps neither in memory (``ValueError``;
    DESIGN.md 3.0)."""
    require_device()
    lib = _lib.load_vort()
    cdt, fdt = _float_code(c, "c", 3), _float_code(f, "f")
    outer, plane, inner = (int(n) for n in c.shape)
    if f.numel() != plane or f.device != c.device:
        raise ValueError(f"f must hold {plane} elements on {c.device}")
    odt = torch.float32 if (cdt, fdt) == (DTYPE_F32, DTYPE_F32) else torch.float64
    out = _out_like(out, (outer, plane, inner), odt, c.device)
    _no_overlap([("out", out)], [("c", c), ("f", f)])
    _call(lib, "mlx_vort_rossby", c.device, _ptr(c), cdt, _ptr(f), fdt, outer, plane, inner,
          _ptr(out))
    return out


# ---------------------------------------------------------------------------------------
# area-weighted means over the plane (include/momlevel_area.h; csrc/momlevel_area.hip)
# ---------------------------------------------------------------------------------------
AREA_MAX_SLOTS = _lib.AREA_MAX_SLOTS  # regions per launch of area_mean
AREA_WINDOW = _lib.AREA_WINDOW  # records a block keeps the maps in registers for


def area_tile(dtype=torch.float64):
    """Cells of the plane one block of mlx_area_mean reduces for a record of ``dtype`` (a torch or
    numpy float32 / float64): the order of summation is a function of this and of the plane."""
    return int(_lib.load_area().mlx_area_tile(_query_dtype(dtype)))


def _area_slot(slot, nslots, plane, device):
    if slot is None:
        if nslots != 1:
            raise ValueError("without a slot map there is one region: nslots must be 1")
        return
    if not (isinstance(slot, torch.Tensor) and slot.is_cuda and slot.dtype == torch.int32
            and slot.dim() == 1 and slot.is_contiguous()):
        raise TypeError("slot must be a contiguous 1-D int32 device tensor")
    if slot.numel() != plane or slot.device != device:
        raise ValueError(f"slot must hold {plane} elements on {device}")


def area_mean(v, area, slot=None, nslots=1):
    """Area-weighted NaN-aware means over the plane (mlx_area_mean): ``v`` (nrec, plane) and
    ``area`` (plane) contiguous device tensors, each float32 or float64 on its own; ``slot`` None
    (one region of every cell) or a (plane) int32 device tensor of slots 0 .. nslots-1, negative =
    no region, with ``nslots`` <= AREA_MAX_SLOTS.  Returns ``(mean, den)``, both (nrec, nslots)
    float64: ``den`` is the valid area under each mean, ``mean`` NaN where it is 0.  Fixed order of
    summation, no atomics: two runs agree to the bit, and a record's means depend on that record
    alone."""
    require_device()
    lib = _lib.load_area()
    vdt, adt = _float_code(v, "v", 2), _float_code(area, "area", 1)
    nrec, plane = (int(n) for n in v.shape)
    if area.numel() != plane or area.device != v.device:
        raise ValueError(f"area must hold {plane} elements on {v.device}")
    nslots = int(nslots)
    if not 1 <= nslots <= AREA_MAX_SLOTS:
        raise ValueError(f"nslots must be 1 .. {AREA_MAX_SLOTS}, got {nslots}: launch in groups")
    _area_slot(slot, nslots, plane, v.device)
    mean = torch.empty((nrec, nslots), dtype=torch.float64, device=v.device)
    den = torch.empty((nrec, nslots), dtype=torch.float64, device=v.device)
    if nrec == 0:
        return mean, den
    if plane == 0:  # numpy: the sum of nothing is 0, 0 / 0 is NaN
        return mean.fill_(float("nan")), den.zero_()
    nbytes = int(lib.mlx_area_mean_workspace_bytes(nrec, plane, nslots, vdt))
    ws = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=v.device)
    _call(lib, "mlx_area_mean", v.device, _ptr(v), vdt, _ptr(area), adt, _ptr(slot), nslots, nrec,
          plane, _ptr(mean), _ptr(den), _ptr(ws), nbytes)
    return mean, den


def area_anomaly(v, mean, slot=None, out=None):
    """``v.astype(float64) - mean[rec, slot]`` (mlx_area_anomaly): ``v`` (nrec, plane) float32 or
    float64, ``mean`` (nrec, nslots) float64, ``slot`` as in area_mean (any number of slots); cells
    of no slot give NaN.  Returns (nrec, plane) float64 (``out`` when given; it must not overlap
    an operand in memory: ``ValueError``)."""
    require_device()
    lib = _lib.load_area()
    vdt = _float_code(v, "v", 2)
    nrec, plane = (int(n) for n in v.shape)
    if (_float_code(mean, "mean", 2) != DTYPE_F64 or int(mean.shape[0]) != nrec
            or mean.device != v.device):
        raise ValueError(f"mean must be a float64 ({nrec}, nslots) tensor on {v.device}")
    nslots = int(mean.shape[1])
    if nslots < 1:
        raise ValueError("mean must hold at least one slot")
    _area_slot(slot, nslots, plane, v.device)
    out = _out_like(out, (nrec, plane), torch.float64, v.device, "float64")
    _no_overlap([("out", out)], [("v", v), ("mean", mean), ("slot", slot)])
    _call(lib, "mlx_area_anomaly", v.device, _ptr(v), vdt, _ptr(slot), nslots, _ptr(mean), nrec,
          plane, _ptr(out))
    return out


# ---------------------------------------------------------------------------------------
# the time Gram matrix behind the EOFs (include/momlevel_eof.h; csrc/momlevel_eof.hip)
# ---------------------------------------------------------------------------------------
GRAM_MAX_SPLIT = _lib.GRAM_MAX_SPLIT  # the most ranges the cells of a time_gram call are cut into


def gram_tile():
    """Rows (and columns) of G one block of mlx_gram_matrix owns (mlx_gram_tile)."""
    return int(_lib.load_eof().mlx_gram_tile())


def gram_cells(n):
    """Cells of one block's range for a record of ``n`` cells (mlx_gram_cells): the partial sums of
    ``ceil(n / gram_cells(n))`` ranges are added in ascending order, so the order of summation is a
    function of ``n`` alone.  0 for n < 1."""
    return int(_lib.load_eof().mlx_gram_cells(int(n)))


def _gram_map(x, n, device, name):
    """a per-cell float64 map of a time_gram call, or None"""
    if x is None:
        return None
    if _float_code(x, name) != DTYPE_F64:
        raise TypeError(f"{name} must be float64")
    if x.numel() != n or x.device != device:
        raise ValueError(f"{name} must hold {n} elements on {device}")
    return x


def time_gram(y1, y2=None, center1=None, center2=None, scale=None):
    """G[s, t] = sum_c b1[s, c] * b2[t, c] with b = (y - center) * scale per cell, 0 in a cell whose
    center1, center2 or scale is NaN (mlx_gram_matrix): ``y1`` (nt1, ...) and ``y2`` (nt2, ...)
    float32 / float64 device records over the same cells, the maps contiguous float64 device
    tensors of one element per cell or None (center 0, scale 1).  Returns a new (nt1, nt2) float64
    device tensor.  ``y2=None`` is the symmetric form (``center2`` must be None too): b2 = b1, the
    tiles above the diagonal computed once, ``G == G.T`` to the bit.  Fixed order of summation on
    the float64 matrix cores, no atomics: two runs agree to the bit, and G[s, t] depends on the rows
    s and t and on the number of cells alone."""
    require_device()
    lib = _lib.load_eof()
    y1, nt1, n, code1 = _time_record(y1)
    dev = y1.device
    if y2 is None:
        if center2 is not None:
            raise ValueError("center2 belongs to y2: the symmetric form takes center1 only")
        nt2, code2, ncols = 0, code1, nt1
    else:
        y2, nt2, n2, code2 = _time_record(y2)
        if n2 != n or y2.device != dev:
            raise ValueError(f"y2 must hold {n} cells a step on {dev}")
        ncols = nt2
    if n < 1:
        raise ValueError("the record holds no cells")
    center1 = _gram_map(center1, n, dev, "center1")
    center2 = _gram_map(center2, n, dev, "center2")
    scale = _gram_map(scale, n, dev, "scale")
    nbytes = int(lib.mlx_gram_matrix_workspace_bytes(nt1, nt2, n))
    if nbytes == 0:
        raise ValueError(f"records of {nt1} and {ncols} steps x {n} cells are outside the Gram "
                         "kernel's range")
    G = torch.empty((nt1, ncols), dtype=torch.float64, device=dev)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    _call(lib, "mlx_gram_matrix", dev, _ptr(y1), code1, _ptr(center1), nt1, _ptr(y2), code2,
          _ptr(center2), nt2, _ptr(scale), n, _ptr(G), _ptr(ws), nbytes)
    return G


def gram_issue_probe(iters=4096, blocks=1024, device="cuda"):
    """Measurement aid: enqueue the issue-rate probe of v_mfma_f64_16x16x4_f64
    (mlx_gram_issue_probe) on ``device``'s current stream; returns the floating-point operations
    of the launch."""
    require_device()
    import ctypes

    device = _indexed(device)
    sink = torch.empty(int(blocks) * 256, dtype=torch.float64, device=device)
    flop = ctypes.c_int64(0)
    _call(_lib.load_eof(), "mlx_gram_issue_probe", device, int(iters), int(blocks), _ptr(sink),
          ctypes.byref(flop))
    return int(flop.value)


# ---------------------------------------------------------------------------------------
# depth-layer sums (include/momlevel_layer.h; csrc/momlevel_layer.hip)
# ---------------------------------------------------------------------------------------
LAYER_MAX = _lib.LAYER_MAX  # layers per launch of layer_integral


def __getattr__(name):
    # LAYER_STEPS is the kernel's own constant: asked of the library on first use, so that
    # importing this module does not need the library
    if name == "LAYER_STEPS":
        return int(_lib.load_layer().mlx_layer_steps())
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def layer_record_blocks(nrec):
    """Block rows along the records of a layer_integral call over ``nrec`` records
    (mlx_layer_record_blocks): ``min(ceil(nrec / LAYER_STEPS), cap)``; past the cap a block goes on
    to further groups of records.  0 for nrec <= 0."""
    return int(_lib.load_layer().mlx_layer_record_blocks(int(nrec)))


def layer_groups(nlayers, cap=LAYER_MAX):
    """``[(start, count)]``: the layers in launches of at most ``cap`` (as regional.slot_groups)"""
    return [(s, min(cap, nlayers - s)) for s in range(0, nlayers, cap)]


def layer_integral(x, z_i, depth, tops, bottoms, surface=None, scale=1.0, out=None):
    """Depth-layer sums (mlx_layer_integral): ``out[r, l, c] = scale * sum_z calc_dz(top[l],
    bottom[l])[z, c] * x[r, z, c]``, NaN terms skipped, z ascending, as tests/layer_numpy.py.

    ``x`` (nrec, nz, plane) contiguous float32 / float64 device tensor; ``z_i`` the nz+1 interfaces;
    ``depth`` (plane), NaN = land; ``tops`` / ``bottoms`` host sequences of equal length, a bottom
    of +inf (or None) meaning the sea floor; ``surface`` None or (plane): NaN there gives NaN.
    Returns (nrec, nl, plane) float64 (``out`` when given; it must not overlap an operand in
    memory: ``ValueError``).  More than LAYER_MAX layers run as
    several launches over groups of layers; every layer gets the bits it would get alone."""
    require_device()
    lib = _lib.load_layer()
    xdt = _float_code(x, "x", 3)
    nrec, nz, plane = (int(n) for n in x.shape)
    dev = x.device
    tops = np.ascontiguousarray(tops, dtype=np.float64).reshape(-1)
    bottoms = np.ascontiguousarray(
        [np.inf if b is None else b for b in np.asarray(bottoms, dtype=object).reshape(-1)],
        dtype=np.float64)
    nl = int(tops.size)
    if nl < 1 or bottoms.size != nl:
        raise ValueError("tops and bottoms must hold the same number (>= 1) of layers")
    z_i = _f64(z_i, dev).reshape(-1)
    depth = _f64(depth, dev).reshape(-1)
    if z_i.numel() != nz + 1 or depth.numel() != plane:
        raise ValueError(f"z_i must have nz+1 = {nz + 1} entries and depth {plane} cells")
    if surface is not None:
        surface = _f64(surface, dev).reshape(-1)
        if surface.numel() != plane:
            raise ValueError(f"surface must hold {plane} cells")
    out = _out_like(out, (nrec, nl, plane), torch.float64, dev, "float64")
    _no_overlap([("out", out)], [("x", x), ("z_i", z_i), ("depth", depth), ("surface", surface)])
    groups = layer_groups(nl)
    for start, count in groups:
        part = out if len(groups) == 1 else torch.empty((nrec, count, plane), dtype=torch.float64,
                                                        device=dev)
        t, b = tops[start:start + count].copy(), bottoms[start:start + count].copy()
        _call(lib, "mlx_layer_integral", dev, _ptr(x), xdt, nrec, nz, plane, _ptr(z_i), _ptr(depth),
              t.ctypes.data, b.ctypes.data, count, _ptr(surface), float(scale), _ptr(part))
        if part is not out:
            out[:, start:start + count] = part
    return out


# ---------------------------------------------------------------------------------------
# the column search (include/momlevel_column.h; csrc/momlevel_column.hip).  EXTENSION.
# ---------------------------------------------------------------------------------------
COLUMN_MAX_TARGETS = _lib.COLUMN_MAX_TARGETS  # targets per launch of column_crossing
COLUMN_MODES = {"rise": _lib.COLUMN_RISE, "fall": _lib.COLUMN_FALL, "depart": _lib.COLUMN_DEPART}
COLUMN_MISS = {"nan": _lib.COLUMN_MISS_NAN, "floor": _lib.COLUMN_MISS_FLOOR}


def column_block_cells(a_dtype=torch.float64, b_dtype=None, generic=False):
    """Cells of the plane one block of column_crossing covers (mlx_column_block_cells) for a field
    of ``a_dtype`` and, SIGMA source, a salinity of ``b_dtype``: 256 packs of 16 bytes of the wider
    field, or 256 single cells on the ``generic`` path."""
    return int(_lib.load_column().mlx_column_block_cells(
        _query_dtype(a_dtype), int(b_dtype is not None),
        _query_dtype(b_dtype) if b_dtype is not None else 0, int(bool(generic))))


def column_record_rows(nrec):
    """Block rows along the records of a column_crossing call over ``nrec`` records
    (mlx_column_record_rows): ``min(nrec, cap)``; past the cap a row goes on to further records.
    0 for nrec <= 0."""
    return int(_lib.load_column().mlx_column_record_rows(int(nrec)))


def column_crossing(a, z, targets, b=None, kref=0, mode="rise", relative=False, miss="nan",
                    floor=None, eos="wright", p_ref=101325.0, out=None):
    """Depth of the first crossing along z (mlx_column_crossing), as tests/column_numpy.py.

    ``a`` (nrec, nz, plane) contiguous float32 / float64 device tensor: the field (FIELD source),
    or theta when ``b``, the salinity of the same shape (its own dtype), is given -- the column
    value is then the float64 density of the widened pair at the scalar pressure ``p_ref`` (SIGMA
    source).  ``z`` the nz level depths; ``targets`` a host sequence; ``kref`` the reference
    level; ``mode`` "rise" | "fall" | "depart"; ``relative``: targets are offsets from the value at
    ``kref``; ``miss`` "nan" | "floor": what a column without a crossing gets (``floor`` (plane)
    when given, else the depth of its deepest level with a value).  Returns (nrec, ntargets,
    plane) float64 (``out`` when given; it must not overlap an operand in memory: ``ValueError``,
    DESIGN.md 3.0).  More than COLUMN_MAX_TARGETS targets run as several
    launches over groups of targets; every target gets the bits it would get alone."""
    require_device()
    lib = _lib.load_column()
    adt = _float_code(a, "a", 3)
    nrec, nz, plane = (int(n) for n in a.shape)
    dev = a.device
    bdt = 0
    if b is not None:
        bdt = _float_code(b, "b", 3)
        if tuple(b.shape) != tuple(a.shape) or b.device != dev:
            raise ValueError("a and b must agree in shape and device")
    try:
        mode_id, miss_id, eos_id = COLUMN_MODES[mode], COLUMN_MISS[miss], EOS_IDS[str(eos).lower()]
    except KeyError as exc:
        raise ValueError(f"unknown mode / miss / eos {exc}") from None
    targets = np.ascontiguousarray(targets, dtype=np.float64).reshape(-1)
    nt = int(targets.size)
    if nt < 1:
        raise ValueError("targets must hold one value at least")
    z = _f64(z, dev).reshape(-1)
    if z.numel() != nz:
        raise ValueError(f"z must have nz = {nz} entries")
    if floor is not None:
        floor = _f64(floor, dev).reshape(-1)
        if floor.numel() != plane:
            raise ValueError(f"floor must hold {plane} cells")
    out = _out_like(out, (nrec, nt, plane), torch.float64, dev, "float64")
    _no_overlap([("out", out)], [("a", a), ("b", b), ("z", z), ("floor", floor)])
    groups = layer_groups(nt, COLUMN_MAX_TARGETS)
    for start, count in groups:
        part = out if len(groups) == 1 else torch.empty((nrec, count, plane), dtype=torch.float64,
                                                        device=dev)
        t = targets[start:start + count].copy()
        _call(lib, "mlx_column_crossing", dev, _ptr(a), adt, _ptr(b), bdt, eos_id, float(p_ref),
              nrec, nz, plane, _ptr(z), int(kref), mode_id, int(bool(relative)), miss_id,
              t.ctypes.data, count, _ptr(floor), _ptr(part))
        if part is not out:
            out[:, start:start + count] = part
    return out


# ---------------------------------------------------------------------------------------
# the time filter (include/momlevel_filter.h; csrc/momlevel_filter.hip).  EXTENSION.
# ---------------------------------------------------------------------------------------
def filter_tile():
    """Output steps a lane of mlx_filter_apply sums together from one pass over its rows: the
    kernel's tile along time (output tiles start at multiples of it)."""
    return int(_lib.load_filter().mlx_filter_tile())


def filter_window_edges():
    """The window lengths at which the kernel's walk over a window changes, ascending
    (mlx_filter_window_edge)."""
    lib = _lib.load_filter()
    edges = []
    while True:
        e = int(lib.mlx_filter_window_edge(len(edges)))
        if e <= 0:
            return tuple(edges)
        edges.append(e)


def filter_tiles_per_block(nt, n, cells_per_lane):
    """Consecutive time tiles one block of mlx_filter_apply walks for an (nt, n) record whose lanes
    hold ``cells_per_lane`` cells (mlx_filter_tiles_per_block); 0 for refused arguments."""
    return int(_lib.load_filter().mlx_filter_tiles_per_block(int(nt), int(n), int(cells_per_lane)))


def filter_weights(w, nt):
    """The host-side mirror of a weight table as the kernel reads it: float64, ``(W,)`` (one row
    for every step) or ``(nt, W)`` (row t for output t), 1 <= W <= nt, every weight finite; or
    ``ValueError``.  Touches no device."""
    w = np.ascontiguousarray(np.asarray(w, dtype=np.float64))
    if w.ndim not in (1, 2) or w.shape[-1] < 1:
        raise ValueError("weights must be (W,) or (nt, W) with W >= 1")
    if w.ndim == 2 and w.shape[0] != int(nt):
        raise ValueError(f"a weight table needs one row per step: ({int(nt)}, W), got {w.shape}")
    if w.shape[-1] > int(nt):
        raise ValueError(f"the window ({w.shape[-1]} steps) is longer than the record ({int(nt)})")
    if not np.isfinite(w).all():
        raise ValueError("weights must be finite")
    return w


def time_filter(y, w, lead, min_count=None, normalise=False, out=None, out_dtype=None):
    """The banded linear operator along the leading axis (mlx_filter_apply):
    ``out[t] = sum_k w[t, k] * y[t - lead + k]``, k = 0 .. W-1 ascending, in float64, as
    tests/filter_numpy.py.  y (nt, ...) float32 / float64 on the device; ``w`` a host array ``(W,)``
    or ``(nt, W)`` (uploaded as float64; non-finite weights are a ``ValueError``) or a float64
    device tensor of one of those shapes (its values are the caller's); ``0 <= lead < W``.  A step
    is valid when it lies in the record and is not NaN; fewer than ``min_count`` (default W) valid
    steps give NaN; ``normalise`` divides by the sum of the valid steps' weights.  Returns
    (nt, ...) of ``out_dtype`` (default y's dtype; float32 is the float64 result rounded once).
    ``out``: a contiguous device tensor of that shape and dtype that overlaps neither y nor device
    weights in memory -- an output step reads W input steps (``ValueError``)."""
    require_device()
    lib = _lib.load_filter()
    y, nt, n, code = _time_record(y)
    if isinstance(w, torch.Tensor) and w.is_cuda:
        if w.dtype != torch.float64 or w.device != y.device or not w.is_contiguous():
            raise ValueError(f"device weights must be a contiguous float64 tensor on {y.device}")
        wd = w
    else:
        wd = hostio.to_device(filter_weights(w, nt), y.device, torch.float64).contiguous()
    if wd.dim() not in (1, 2) or (wd.dim() == 2 and wd.shape[0] != nt):
        raise ValueError(f"weights must be (W,) or ({nt}, W)")
    W = int(wd.shape[-1])
    if not 1 <= W <= nt:
        raise ValueError(f"the window must hold 1 .. {nt} steps, got {W}")
    lead = int(lead)
    if not 0 <= lead < W:
        raise ValueError(f"lead must lie in [0, {W}), got {lead}")
    min_count = W if min_count is None else int(min_count)
    if not 1 <= min_count <= W:
        raise ValueError(f"min_count must lie in [1, {W}], got {min_count}")
    out_dtype = y.dtype if out_dtype is None else out_dtype
    if out_dtype not in (torch.float32, torch.float64):
        raise TypeError(f"out_dtype must be float32 or float64, got {out_dtype}")
    out = _out_like(out, tuple(y.shape), out_dtype, y.device)
    _no_overlap([("out", out)], [("y", y), ("w", wd)])
    if n == 0:
        return out
    _call(lib, "mlx_filter_apply", y.device, _ptr(y), code, _ptr(wd), W, W if wd.dim() == 2 else 0,
          lead, min_count, _lib.FILTER_NORMALISE if normalise else 0, nt, n, _ptr(out),
          DTYPE_F64 if out_dtype == torch.float64 else DTYPE_F32)
    return out


# ---------------------------------------------------------------------------------------
# the horizontal filter (include/momlevel_smooth.h; csrc/momlevel_smooth.hip).  EXTENSION.
# ---------------------------------------------------------------------------------------
def smooth_tile(dtype=torch.float64):
    """``(tile_h, tile_w)``: the output cells one block of mlx_smooth_apply's tiled path owns for a
    record of ``dtype`` (a torch or numpy float32 / float64).  The results do not depend on it."""
    lib = _lib.load_smooth()
    return int(lib.mlx_smooth_tile_h()), int(lib.mlx_smooth_tile_w(_query_dtype(dtype)))


def smooth_max_window():
    """The largest Wx and Wy the tiled path takes (mlx_smooth_max_window); wider windows are summed
    cell by cell, with the same bits."""
    return int(_lib.load_smooth().mlx_smooth_max_window())


def smooth_record_window():
    """Records a block of the tiled path walks while it holds its maps (mlx_smooth_record_window)."""
    return int(_lib.load_smooth().mlx_smooth_record_window())


def smooth_record_rows(nrec):
    """Block rows along the records of a call of ``nrec`` records that goes cell by cell
    (mlx_smooth_record_rows): ``min(nrec, cap)``; past the cap a row goes on to further records.
    The results do not depend on it."""
    return int(_lib.load_smooth().mlx_smooth_record_rows(int(nrec)))


def smooth_tiled(Wx, Wy, ny, nx):
    """1 when a call of a ``Wy`` x ``Wx`` window on a ``(ny, nx)`` plane takes the tiled path, given
    ``v`` and ``out`` on 16-byte boundaries (mlx_smooth_tiled); 0 when it goes cell by cell, and
    for extents that mlx_smooth_apply refuses.  The results do not depend on it."""
    return int(_lib.load_smooth().mlx_smooth_tiled(int(Wx), int(Wy), int(ny), int(nx)))


def smooth_weights(wx, wy, ny, nx):
    """The host-side mirror of the weights as the kernel reads them: float64, ``wx`` ``(Wx,)`` (one
    row for every source row) or ``(ny, Wx)`` (row r for source row r), ``wy`` ``(Wy,)``,
    1 <= Wx <= nx, 1 <= Wy <= ny, every weight finite; or ``ValueError``.  Touches no device."""
    wx = np.ascontiguousarray(np.asarray(wx, dtype=np.float64))
    wy = np.ascontiguousarray(np.asarray(wy, dtype=np.float64))
    if wx.ndim not in (1, 2) or wx.shape[-1] < 1:
        raise ValueError("x weights must be (Wx,) or (ny, Wx) with Wx >= 1")
    if wx.ndim == 2 and wx.shape[0] != int(ny):
        raise ValueError(f"a table of x weights needs one row per row of the plane: ({int(ny)}, Wx), "
                         f"got {wx.shape}")
    if wy.ndim != 1 or wy.shape[0] < 1:
        raise ValueError("y weights must be (Wy,) with Wy >= 1")
    if wx.shape[-1] > int(nx) or wy.shape[0] > int(ny):
        raise ValueError(f"the window ({wy.shape[0]} x {wx.shape[-1]} cells) is larger than the "
                         f"plane ({int(ny)} x {int(nx)}): a periodic window may not lap itself")
    if not (np.isfinite(wx).all() and np.isfinite(wy).all()):
        raise ValueError("weights must be finite")
    return wx, wy


def plane_smooth(v, area, wx, wy, lead_x, lead_y, periodic_x, min_count, fill=False, residual=False,
                 out_dtype=None):
    """The separable, normalised, mask-aware convolution over the two trailing dims
    (mlx_smooth_apply; include/momlevel_smooth.h states the contract, tests/smooth_numpy.py restates
    it): ``v`` (nrec, ny, nx) and ``area`` (ny, nx) contiguous device tensors, each float32 or
    float64 on its own; ``wx`` a host array ``(Wx,)`` or ``(ny, Wx)`` and ``wy`` ``(Wy,)`` (uploaded
    as float64; non-finite weights are a ``ValueError``) or float64 device tensors of those shapes
    (their values are the caller's); ``0 <= lead < W`` each way.  A cell is valid when neither its
    value nor its area is NaN and its area is positive; x wraps with ``periodic_x``, the y edges
    are closed.  Fewer than ``min_count`` valid cells in the window give NaN, and so does a centre
    that is not valid unless ``fill``; ``residual`` returns ``v - smooth``.  Returns
    a new (nrec, ny, nx) tensor of ``out_dtype`` (default v's dtype; float32 is the float64 result
    rounded once).  It takes no result buffer: the table of entry points that do is closed
    (tests/test_gpu_out_contract.py); mlx_smooth_apply itself refuses an out that overlaps an
    operand, and tests/test_gpu_smooth_edges.py runs it into guard-banded views."""
    require_device()
    lib = _lib.load_smooth()
    vdt, adt = _float_code(v, "v", 3), _float_code(area, "area", 2)
    nrec, ny, nx = (int(n) for n in v.shape)
    if tuple(area.shape) != (ny, nx) or area.device != v.device:
        raise ValueError(f"area must be ({ny}, {nx}) on {v.device}")
    if ny < 1 or nx < 1:
        raise ValueError("the plane must hold at least one cell")
    dev_w = [isinstance(w, torch.Tensor) and w.is_cuda for w in (wx, wy)]
    if dev_w[0] != dev_w[1]:
        raise ValueError("wx and wy must both be host arrays or both device tensors")
    if dev_w[0]:
        for name, w in (("wx", wx), ("wy", wy)):
            if w.dtype != torch.float64 or w.device != v.device or not w.is_contiguous():
                raise ValueError(f"device weights ({name}) must be a contiguous float64 tensor on "
                                 f"{v.device}")
        wxd, wyd = wx, wy
    else:
        hx, hy = smooth_weights(wx, wy, ny, nx)
        wxd = hostio.to_device(hx, v.device, torch.float64).contiguous()
        wyd = hostio.to_device(hy, v.device, torch.float64).contiguous()
    if wxd.dim() not in (1, 2) or (wxd.dim() == 2 and wxd.shape[0] != ny) or wyd.dim() != 1:
        raise ValueError(f"weights must be wx (Wx,) or ({ny}, Wx) and wy (Wy,)")
    Wx, Wy = int(wxd.shape[-1]), int(wyd.shape[0])
    if not (1 <= Wx <= nx and 1 <= Wy <= ny):
        raise ValueError(f"the window must hold 1 .. {ny} by 1 .. {nx} cells, got {Wy} x {Wx}")
    lead_x, lead_y = int(lead_x), int(lead_y)
    if not (0 <= lead_x < Wx and 0 <= lead_y < Wy):
        raise ValueError(f"leads must lie in [0, {Wx}) and [0, {Wy}), got {lead_x} and {lead_y}")
    min_count = int(min_count)
    if not 1 <= min_count <= Wx * Wy:
        raise ValueError(f"min_count must lie in [1, {Wx * Wy}], got {min_count}")
    out_dtype = v.dtype if out_dtype is None else out_dtype
    if out_dtype not in (torch.float32, torch.float64):
        raise TypeError(f"out_dtype must be float32 or float64, got {out_dtype}")
    out = torch.empty((nrec, ny, nx), dtype=out_dtype, device=v.device)
    if nrec == 0:
        return out
    flags = (_lib.SMOOTH_FILL if fill else 0) | (_lib.SMOOTH_RESIDUAL if residual else 0)
    _call(lib, "mlx_smooth_apply", v.device, _ptr(v), vdt, _ptr(area), adt, _ptr(wxd), Wx,
          Wx if wxd.dim() == 2 else 0, lead_x, _ptr(wyd), Wy, lead_y, int(bool(periodic_x)),
          min_count, flags, nrec, ny, nx, _ptr(out),
          DTYPE_F64 if out_dtype == torch.float64 else DTYPE_F32)
    return out


# ---------------------------------------------------------------------------------------
# the grid-to-grid remap (include/momlevel_regrid.h; csrc/momlevel_regrid.hip).  EXTENSION.
# ---------------------------------------------------------------------------------------
def regrid_slice():
    """Destinations of one slice of the remap table (mlx_regrid_slice): one wave owns a slice, one
    lane a destination.  The results do not depend on it; the packed layout does."""
    return int(_lib.load_regrid().mlx_regrid_slice())


def regrid_record_window():
    """Records a block walks on one read of its table entries (mlx_regrid_record_window)."""
    return int(_lib.load_regrid().mlx_regrid_record_window())


def regrid_window_rows(nrec):
    """Block rows along the records of a call of ``nrec`` records (mlx_regrid_window_rows):
    ``min(ceil(nrec / regrid_record_window()), cap)``; past the cap a row goes on to further
    windows of records.  The results do not depend on it."""
    return int(_lib.load_regrid().mlx_regrid_window_rows(int(nrec)))


def regrid_apply(v, plan_tensors, nsrc, ndst, min_frac=0.0, propagate=False, renorm=True,
                 out_dtype=None):
    """The remap through a sparse weight table (mlx_regrid_apply; include/momlevel_regrid.h states
    the contract and the packed layout, tests/regrid_numpy.py restates both): ``v`` (nrec, nsrc) a
    contiguous float32 or float64 device tensor; ``plan_tensors`` = ``(slice_ptr, len, col, S)``,
    contiguous 1-D device tensors on v's device -- int64 ``(ceil(ndst / regrid_slice()) + 1,)``,
    int32 ``(ndst,)``, int32 ``(nentries,)`` and float64 ``(nentries,)`` (their values are the
    caller's: whatever they hold, the kernel reads nothing outside them).  Sources that are NaN are
    left out and the weights present renormalised (``renorm=False``: not renormalised); a
    destination whose valid weight is below ``min_frac`` of its whole weight, or without a valid
    source, is NaN; ``propagate`` makes any NaN source a NaN result instead.  Returns a new
    (nrec, ndst) tensor of ``out_dtype`` (default v's dtype; float32 is the float64 result rounded
    once).  It takes no result buffer: the table of entry points that do is closed
    (tests/test_gpu_out_contract.py); mlx_regrid_apply itself refuses an out that overlaps an
    operand, and tests/test_gpu_regrid_edges.py runs it into guard-banded views."""
    require_device()
    lib = _lib.load_regrid()
    vdt = _float_code(v, "v", 2)
    nrec, nsrc, ndst = int(v.shape[0]), int(nsrc), int(ndst)
    if nsrc < 0 or ndst < 0 or int(v.shape[1]) != nsrc:
        raise ValueError(f"v must be (nrec, {nsrc}), got {tuple(v.shape)}")
    if nsrc >= 2 ** 31:
        raise ValueError("the source plane must hold fewer than 2^31 cells")
    try:
        slice_ptr, length, col, S = plan_tensors
    except (TypeError, ValueError):
        raise ValueError("plan_tensors must be (slice_ptr, len, col, S)") from None
    for name, t, dt in (("slice_ptr", slice_ptr, torch.int64), ("len", length, torch.int32),
                        ("col", col, torch.int32), ("S", S, torch.float64)):
        if not (isinstance(t, torch.Tensor) and t.dtype == dt and t.dim() == 1 and t.is_contiguous()
                and t.device == v.device):
            raise ValueError(f"{name} must be a contiguous 1-D {dt} tensor on {v.device}")
    nslices = -(-ndst // regrid_slice())
    if slice_ptr.shape[0] != nslices + 1 or length.shape[0] != ndst or col.shape[0] != S.shape[0]:
        raise ValueError(f"the table of {ndst} destinations needs slice_ptr ({nslices + 1},), len "
                         f"({ndst},) and col and S of one length")
    min_frac = float(min_frac)
    if not 0.0 <= min_frac <= 1.0:  # (a NaN compares false)
        raise ValueError(f"min_frac must lie in [0, 1], got {min_frac}")
    out_dtype = v.dtype if out_dtype is None else out_dtype
    if out_dtype not in (torch.float32, torch.float64):
        raise TypeError(f"out_dtype must be float32 or float64, got {out_dtype}")
    out = torch.empty((nrec, ndst), dtype=out_dtype, device=v.device)
    if nrec == 0 or ndst == 0:
        return out
    flags = (_lib.REGRID_PROPAGATE if propagate else 0) | (0 if renorm else _lib.REGRID_NO_RENORM)
    _call(lib, "mlx_regrid_apply", v.device, _ptr(v), vdt, _ptr(slice_ptr), _ptr(length), _ptr(col),
          _ptr(S), int(S.shape[0]), min_frac, flags, nrec, nsrc, ndst, _ptr(out),
          DTYPE_F64 if out_dtype == torch.float64 else DTYPE_F32)
    return out


# ---------------------------------------------------------------------------------------
# the census (include/momlevel_census.h; csrc/momlevel_census.hip).  EXTENSION.
# ---------------------------------------------------------------------------------------
def census_tile():
    """Cells of one tile of the census (mlx_census_tile): a thread owns four consecutive cells."""
    return int(_lib.load_census().mlx_census_tile())


def census_blocks(ncells):
    """Blocks that share one record of ``ncells`` cells (mlx_census_blocks): a pure function of
    ``ncells``, and with it the order of summation."""
    return int(_lib.load_census().mlx_census_blocks(int(ncells)))


def census_max_bins(nfields=1, has_weights=False, has_values=False):
    """The most bins of one launch (mlx_census_max_bins): larger tables go in bin groups."""
    return int(_lib.load_census().mlx_census_max_bins(int(nfields), int(bool(has_weights)),
                                                      int(bool(has_values))))


def census_workspace_bytes(nrec, ncells, nbins, has_weights=False, has_values=False):
    """Bytes of partials one launch needs (mlx_census_workspace_bytes)."""
    return int(_lib.load_census().mlx_census_workspace_bytes(
        int(nrec), int(ncells), int(nbins), int(bool(has_weights)), int(bool(has_values))))


def census(fields, edges, weights=None, values=None, closed=3):
    """One launch of the census (mlx_census_histogram; include/momlevel_census.h states the
    contract, tests/census_numpy.py restates it): ``fields`` one or two (nrec, ncells) contiguous
    float32 / float64 device tensors, ``edges`` one contiguous 1-D float64 device tensor of
    ``n_d + 1`` edges per field (their values are the caller's: whatever they hold, the kernel
    writes nothing outside its tables), ``weights`` None, (ncells,) or (nrec, ncells), ``values``
    None or (nrec, ncells) and only with weights.  ``closed``: bit d set when a value on the last
    edge of field d belongs to its last bin (3 for a whole table; a bin group clears the bit of a
    field whose last edge is not the table's).  Returns ``(count, wsum, vsum)``: (nrec, nbins) int64
    and float64 tensors, nbins = n_0 (* n_1), ``wsum`` / ``vsum`` None without weights / values.
    More bins than ``census_max_bins`` are a ``ValueError``: launch in groups
    (momlevel_amd/census.py).  It takes no result buffer, as ``regrid_apply``; the results are new
    tensors, checked against the operands like every other result."""
    require_device()
    lib = _lib.load_census()
    fields, edges = tuple(fields), tuple(edges)
    D = len(fields)
    if D not in (1, 2) or len(edges) != D:
        raise ValueError("the census bins by one or two fields, with one edge array each")
    codes = [_float_code(f, f"fields[{d}]", 2) for d, f in enumerate(fields)]
    dev = fields[0].device
    nrec, ncells = (int(n) for n in fields[0].shape)
    if D == 2 and (tuple(fields[1].shape) != (nrec, ncells) or fields[1].device != dev):
        raise ValueError(f"fields[1] must be ({nrec}, {ncells}) on {dev}")
    for d, e in enumerate(edges):
        if not (isinstance(e, torch.Tensor) and e.dtype == torch.float64 and e.dim() == 1
                and e.is_contiguous() and e.device == dev and e.numel() >= 2):
            raise ValueError(f"edges[{d}] must be a contiguous 1-D float64 tensor of at least two "
                             f"edges on {dev}")
    n = [int(e.numel()) - 1 for e in edges] + [1] * (2 - D)
    nbins = n[0] * n[1]
    if values is not None and weights is None:
        raise ValueError("values need weights: the sum is of weights * values")
    cap = census_max_bins(D, weights is not None, values is not None)
    if nbins > cap:
        raise ValueError(f"{nbins} bins are more than the {cap} of one launch: launch in bin groups")
    wdt = vdt = DTYPE_F64
    per_record = 0
    if weights is not None:
        wdt = _float_code(weights, "weights")
        per_record = int(weights.dim() == 2)
        if tuple(weights.shape) not in ((ncells,), (nrec, ncells)) or weights.device != dev:
            raise ValueError(f"weights must be ({ncells},) or ({nrec}, {ncells}) on {dev}")
    if values is not None:
        vdt = _float_code(values, "values", 2)
        if tuple(values.shape) != (nrec, ncells) or values.device != dev:
            raise ValueError(f"values must be ({nrec}, {ncells}) on {dev}")
    if int(closed) not in (0, 1, 2, 3):
        raise ValueError(f"closed must be 0 .. 3, got {closed}")
    count = _out_like(None, (nrec, nbins), torch.int64, dev)
    wsum = None if weights is None else _out_like(None, (nrec, nbins), torch.float64, dev)
    vsum = None if values is None else _out_like(None, (nrec, nbins), torch.float64, dev)
    if nrec == 0:
        return count, wsum, vsum
    if ncells == 0:  # numpy: the sum of nothing is 0
        return count.zero_(), None if wsum is None else wsum.zero_(), \
            None if vsum is None else vsum.zero_()
    nbytes = census_workspace_bytes(nrec, ncells, nbins, weights is not None, values is not None)
    if nbytes == 0:
        raise ValueError(f"a census of {nrec} records of {ncells} cells is more than one launch "
                         "takes: window the records")
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
    _no_overlap([("count", count), ("wsum", wsum), ("vsum", vsum), ("workspace", ws)],
                [(f"fields[{d}]", f) for d, f in enumerate(fields)]
                + [(f"edges[{d}]", e) for d, e in enumerate(edges)]
                + [("weights", weights), ("values", values)])
    _call(lib, "mlx_census_histogram", dev, _ptr(fields[0]), codes[0],
          _ptr(fields[1]) if D == 2 else None, codes[1] if D == 2 else DTYPE_F64, D,
          _ptr(edges[0]), n[0], _ptr(edges[1]) if D == 2 else None, n[1], int(closed),
          _ptr(weights), wdt, per_record, _ptr(values), vdt, nrec, ncells, _ptr(count),
          _ptr(wsum), _ptr(vsum), _ptr(ws), nbytes)
    return count, wsum, vsum


# ---------------------------------------------------------------------------------------
# order statistics (include/momlevel_quantile.h; csrc/momlevel_quantile.hip).  EXTENSION.
# ---------------------------------------------------------------------------------------
def quantile_block_cells(dtype=torch.float64):
    """Cells one block of the quantile kernels' pack path covers (mlx_quantile_block_cells)."""
    return int(_lib.load_quantile().mlx_quantile_block_cells(_query_dtype(dtype)))


def quantile_unroll():
    """Rows of a group a lane of the quantile kernels has in flight (mlx_quantile_unroll)."""
    return int(_lib.load_quantile().mlx_quantile_unroll())


def quantile_levels(q):
    """``q`` as the kernel takes it: a 1-D float64 host array of at least one level, each in
    [0, 1]; or ``ValueError``.  Touches no device."""
    try:
        levels = np.asarray(q, dtype=np.float64)
    except (TypeError, ValueError) as exc:
        raise ValueError(f"q must be a number or a sequence of numbers in [0, 1], got {q!r}") from exc
    if levels.ndim > 1 or levels.size < 1:
        raise ValueError("q must be a number or a 1-D sequence of at least one number")
    levels = np.ascontiguousarray(levels.reshape(-1))
    if not np.all((levels >= 0.0) & (levels <= 1.0)):  # (false for NaN)
        raise ValueError(f"every q must lie in [0, 1], got {q!r}")
    return levels


def _quantile_groups(nt, y, steps, offsets):
    """(steps ptr, offsets ptr, nsel, ngroups, keep-alive) of a quantile call: a ``DeviceGroups``,
    host lists (checked, uploaded), or None for all rows in order"""
    if steps is None:
        if offsets is not None:
            raise ValueError("offsets without steps")
        return None, None, nt, 1, None
    if isinstance(steps, DeviceGroups):
        groups = steps
        if offsets is not None:
            raise ValueError("a DeviceGroups carries its own offsets")
        if groups.nt != nt or groups.steps.device != y.device:
            raise ValueError("the groups were made for another record length or device")
    else:
        groups = DeviceGroups(steps, offsets, nt, y.device)
    return _ptr(groups.steps), _ptr(groups.offsets), groups.nsel, groups.ngroups, groups


def time_quantile(y, q, steps=None, offsets=None, out=None):
    """NaN-skipping quantiles along the leading axis (mlx_quantile_select): y (nt, ...) float32 /
    float64 on the device, ``q`` one level or a sequence of levels in [0, 1]  ->
    (nq, ngroups, ...) of y's dtype.  Groups as in ``time_group_stat`` (host lists or a
    ``DeviceGroups``); ``steps`` None: one group of all rows.  float64 results are value-identical
    to ``numpy.nanquantile(y[sel], q, axis=0)`` (tests/quantile_numpy.py restates the contract);
    float32 records are selected and interpolated in float64 and rounded once.  Any number of
    levels: the kernel takes ``QUANTILE_MAX_Q`` a launch.  ``out``: a contiguous device tensor of
    the result's shape and dtype that overlaps no operand in memory (``ValueError``; DESIGN.md
    3.0)."""
    require_device()
    lib = _lib.load_quantile()
    levels = quantile_levels(q)
    y, nt, n, code = _time_record(y)
    sp, op, nsel, ngroups, _keep = _quantile_groups(nt, y, steps, offsets)
    shape = (int(levels.size), ngroups) + tuple(y.shape[1:])
    out = _out_like(out, shape, y.dtype, y.device)
    _no_overlap([("out", out)], [("y", y), ("steps", getattr(_keep, "steps", None)),
                                 ("offsets", getattr(_keep, "offsets", None))])
    if n == 0:
        return out
    for c0 in range(0, levels.size, _lib.QUANTILE_MAX_Q):
        chunk = np.ascontiguousarray(levels[c0:c0 + _lib.QUANTILE_MAX_Q])
        _call(lib, "mlx_quantile_select", y.device, _ptr(y), code, sp, op, nsel, ngroups, nt, n,
              chunk.ctypes.data, int(chunk.size), _ptr(out[c0:c0 + chunk.size]))
    return out


def time_exceed_count(y, thr, steps=None, offsets=None):
    """Steps of each group with ``y > thr`` (mlx_quantile_exceed_count): strict, compared in
    float64, a NaN on either side counts nothing.  y (nt, ...) float32 / float64 on the device,
    ``thr`` (ngroups, ...) (any float dtype, used as float64), groups as in ``time_quantile``  ->
    (ngroups, ...) int64."""
    require_device()
    lib = _lib.load_quantile()
    y, nt, n, code = _time_record(y)
    sp, op, nsel, ngroups, _keep = _quantile_groups(nt, y, steps, offsets)
    shape = (ngroups,) + tuple(y.shape[1:])
    thr = _f64(thr, y.device)
    if tuple(thr.shape) != shape:
        raise ValueError(f"thr must have shape {shape} (one row per group), got {tuple(thr.shape)}")
    out = torch.empty(shape, dtype=torch.int64, device=y.device)
    if n == 0:
        return out
    _call(lib, "mlx_quantile_exceed_count", y.device, _ptr(y), code, sp, op, nsel, ngroups, nt, n,
          _ptr(thr), _ptr(out))
    return out


def calc_dz(z_i, depth, top=0.0, bottom=None, fraction=False):
    """derived.calc_dz core on device -> (nz, ny, nx)."""
    require_device()
    depth = _f64(depth, depth.device if isinstance(depth, torch.Tensor) else "cuda")
    z_i = _f64(z_i, depth.device)
    nz = z_i.numel() - 1
    ny, nx = depth.shape
    out = torch.empty((nz, ny, nx), dtype=torch.float64, device=depth.device)
    _call(_lib.load(), "mlx_calc_dz", depth.device, _ptr(z_i), _ptr(depth), nz, ny * nx, float(top),
          float(bottom) if bottom is not None else 0.0, int(bottom is not None),
          int(bool(fraction)), _ptr(out))
    return out


def synth_field(shape, dtype=torch.float64, *, seed, field_id, lo, scale, mask3d=None,
                t0=0, global_hw=None, origin=(0, 0), device="cuda", out=None):
    """Counter-based synthetic field (bench / full-size tests); see synthetic.py.  ``out``: a
    contiguous tensor of exactly ``shape``, ``dtype`` and ``device`` that does not overlap
    ``mask3d`` in memory (``ValueError``)."""
    require_device()
    nt, nz, ny, nx = (int(v) for v in shape)
    NY, NX = global_hw if global_hw is not None else (ny, nx)
    if dtype not in (torch.float32, torch.float64):
        raise TypeError(f"dtype must be float32 or float64, got {dtype}")
    out = _out_like(out, (nt, nz, ny, nx), dtype, device)
    code = DTYPE_F64 if dtype == torch.float64 else DTYPE_F32
    if mask3d is not None:
        mask3d = _f64(mask3d, out.device)
    _no_overlap([("out", out)], [("mask3d", mask3d)])
    _call(_lib.load(), "mlx_synth_field", out.device, _ptr(out), code, nt, nz, ny, nx, t0, NY, NX,
          origin[0], origin[1], seed, field_id, float(lo), float(scale), _ptr(mask3d))
    return out
