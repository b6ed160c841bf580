"""flament.py -- P. Flament (2002) spiciness on the HIP kernel (mlx_spice_map).

Same call as the reference's ``momlevel.spice.flament.spice`` (src/momlevel/spice/flament.py:43-95):
host arrays are uploaded, evaluated on the MI355X and copied back; device tensors stay on the
device.  There is no host arithmetic fallback.

Flament, P. 2002: A state variable for characterizing water masses and their diffusive stability:
spiciness.  Progress in Oceanography, 54, 493-501.  https://doi.org/10.1016/S0079-6611(02)00065-4

The result is float64 for every input dtype, as in numpy.  Its bits are NOT numpy's: the reference
takes the powers with libm's pow (float32 powers of float32 fields) and sums 30 products, the
kernel nests 29 fmas in float64 (include/momlevel_spice.h); the difference is bounded, see
DESIGN.md 3.11.  ``MOMLEVEL_AMD_F32_MODE`` does not apply.
"""

import numpy as np
import torch

from .. import core, hostio
from ..eos import _dispatch
from ..labeled import is_lazy

__all__ = ["spice"]


def _on_device(thetao, so, device):
    """the map on two operands of one shape (arrays or tensors)  ->  a device tensor of that shape"""
    T, S = _dispatch._as_tensor(thetao, device), _dispatch._as_tensor(so, device)
    shape = tuple(T.shape)
    out = core.spice_map(T.contiguous().reshape(-1), S.contiguous().reshape(-1))
    return out.reshape(shape)


def spice(thetao, so):
    """Seawater spiciness after Flament (2002).

    Parameters
    ----------
    thetao : numpy.ndarray or torch.Tensor
        Sea water potential temperature in deg C
    so : numpy.ndarray or torch.Tensor
        Sea water practical salinity in PSU

    Returns
    -------
    numpy.ndarray or torch.Tensor
        Sea water spiciness, unitless: float64, of the inputs' shape; a tensor on the inputs'
        device when one of them is a device tensor, a numpy array otherwise
    """
    core.require_device()
    # python numbers become one-element arrays (flament.py:68-70; np.float64 is a float)
    thetao = np.array([float(thetao)]) if isinstance(thetao, (float, int)) else thetao
    so = np.array([float(so)]) if isinstance(so, (float, int)) else so
    # a numpy masked array (a netCDF4 read) means NaN where it is masked
    thetao, so = (hostio.as_plain(x) if isinstance(x, np.ma.MaskedArray) else x for x in (thetao, so))
    if not all(isinstance(x, torch.Tensor) or is_lazy(x) for x in (thetao, so)):
        thetao, so = (x if isinstance(x, torch.Tensor) or is_lazy(x) else np.asarray(x)
                      for x in (thetao, so))
    shape = _dispatch._shape(thetao)
    assert shape == _dispatch._shape(so), "thetao and so must have the same shape"
    for x in (thetao, so):
        _dispatch._kind(x)  # float16 / long double are refused; integers compute as float64

    tensors = [x for x in (thetao, so) if isinstance(x, torch.Tensor)]
    if not tensors:
        if len(shape) >= 1 and hostio.wants_pipeline(shape[0], int(np.prod(shape))):
            device = torch.device("cuda", torch.cuda.current_device())
            return _dispatch._host_pipeline(
                [thetao, so], lambda ops: _on_device(ops[0], ops[1], device))
        thetao, so = (hostio.as_plain(x[...]) if is_lazy(x) else x for x in (thetao, so))
    device = next((x.device for x in tensors if x.is_cuda),
                  torch.device("cuda", torch.cuda.current_device()))
    out = _on_device(thetao, so, device)
    if any(x.is_cuda for x in tensors):
        return out
    return hostio.to_host(out)
