"""The library's own dense linear algebra on the device (C ABI: m3g_eigh_batched, csrc/m3g_eigh.hip).

`eigh_batched` stands where `numpy.linalg.eigh` / `torch.linalg.eigh` would over a batch of small Hermitian matrices: cyclic Jacobi
with complex rotations in fp64, one workgroup per matrix, matrix and eigenvectors in LDS.  A matrix's outputs have the same bits
alone, at any position of a batch and for any batch size."""
from __future__ import annotations

import torch

from . import _cuda, _lib
from ._driver import check_tensor
from .data.graph_gpu import _ptr, _stream

EIGH_MAX_N = _lib.EIGH_MAX_N


def eigh_batched(a: torch.Tensor, eigenvectors: bool = True):
    """Eigenvalues `w` [..., n] (float64, ascending, ties in index order), eigenvectors `v` [..., n, n] (complex128, column k
    belonging to eigenvalue k; None with eigenvectors=False -- the eigenvalues have the same bits either way) and `info` [...]
    (int32: sweeps run in the bits `_lib.EIGH_SWEEPS_MASK`, `_lib.EIGH_NONFINITE` / `_lib.EIGH_NOT_CONVERGED` above them) of the
    Hermitian matrices `a` [..., n, n], complex128 or float64 (real symmetric), contiguous, on a GPU.  Only the upper triangle and
    the real part of the diagonal are read.  A flagged matrix gets NaN; the others are unaffected.  n <= EIGH_MAX_N.  Queued on the
    current stream: no wait (a float64 input is widened to complex128 by a torch op first)."""
    if not torch.is_tensor(a) or a.dim() < 2 or a.shape[-1] != a.shape[-2] or a.dtype not in (torch.complex128, torch.float64):
        raise ValueError("a must be a [..., n, n] complex128 or float64 tensor")
    if not isinstance(eigenvectors, bool):
        raise ValueError(f"eigenvectors must be True or False; got {eigenvectors!r}")
    n = int(a.shape[-1])
    if n < 1:
        raise ValueError("a must be a [..., n, n] tensor with n >= 1")
    if n > EIGH_MAX_N:
        raise ValueError(f"eigh_batched: n = {n} is above EIGH_MAX_N = {EIGH_MAX_N}")
    if a.device.type != "cuda":
        raise ValueError(f"eigh_batched runs on a GPU device; got {a.device}")
    check_tensor("a", a, tuple(a.shape), a.dtype, a.device)   # contiguous
    batch = tuple(a.shape[:-2])
    z = a.to(torch.complex128).reshape(-1, n, n)
    m = z.shape[0]
    w = torch.empty(m, n, dtype=torch.float64, device=a.device)
    v = torch.empty(m, n, n, dtype=torch.complex128, device=a.device) if eigenvectors else None
    info = torch.empty(m, dtype=torch.int32, device=a.device)
    if m:
        lib = _lib.load_library()
        with _cuda.on_device(a.device):
            _lib.check(lib.m3g_eigh_batched(m, n, _ptr(z), 1 if eigenvectors else 0, _ptr(w), _ptr(v) if eigenvectors else None, _ptr(info),
                                            _stream()))
    return w.reshape(batch + (n,)), (v.reshape(batch + (n, n)) if eigenvectors else None), info.reshape(batch)
