"""Typed wrappers over the C ABI: the one place a tensor becomes the argument list of ``lpf_gemm_f32``,
``lpf_layernorm_f32``, ``lpf_pair_gather_f32`` or ``lpf_spmm_csr_*``, and the one definition of what those launches
need around them -- the raw stream, the row layout, the hub-row list.

Two rules keep a recorded plan (``PlannedScorer``, ``_lib.recording``) complete: every wrapper fetches the library
with ``_lib.hip()`` AT CALL TIME, and every address goes through ``_lib.ptr``.

``tag``: the ``KernelTimer`` span around the launch; None opens none.
"""
from __future__ import annotations

import torch

from . import _lib
from ._lib import FLAG_RELU, check, ptr
from .profile import _NOOP, KernelTimer


def _span(tag):
    return _NOOP if tag is None else KernelTimer.span(tag)


def raw_stream(dev) -> int:
    """The current raw HIP stream of ``dev`` (a ``torch.device``; no index: the current device) -- the stream every
    C-ABI launch goes to."""
    return torch._C._cuda_getCurrentRawStream(dev.index if dev.index is not None else torch.cuda.current_device())


def pad4(k: int) -> int:
    return (k + 3) & ~3


def f32_rows(x: torch.Tensor) -> torch.Tensor:
    """``x`` detached, fp32, 2-D, inner stride 1, row stride a multiple of 4 floats and 16-byte aligned (what
    lpf_gemm_f32 wants); a zero-padded copy only when needed."""
    if x.requires_grad:
        x = x.detach()
    if x.dtype != torch.float32:
        x = x.float()
    if x.dim() != 2:
        x = x.reshape(-1, x.shape[-1])
    if x.stride(1) != 1 or x.stride(0) % 4 or x.data_ptr() % 16 or x.stride(0) < x.shape[1]:
        k = x.shape[1]
        buf = torch.zeros(x.shape[0], pad4(k), dtype=torch.float32, device=x.device)
        buf[:, :k] = x
        x = buf[:, :k]
    return x


def gemm(a: torch.Tensor, w: torch.Tensor, bias=None, addend=None, relu=False, out=None, tag=None) -> torch.Tensor:
    """out = a [M, K] @ w [N, K]^T (+ bias) (+ addend) (ReLU) through ``lpf_gemm_f32`` (bias, addend and ReLU ride in
    the kernel's epilogue).  ``out``: a strided view with 16-byte aligned rows; without one the result's rows are
    padded to 4 floats."""
    if not a.is_cuda:
        raise _lib.LpfError(f"gemm: tensors must live on an MI355X (got {a.device}); lpformer_amd has no CPU fallback")
    a, w = f32_rows(a), f32_rows(w)
    m, k = a.shape
    n = w.shape[0]
    assert w.shape[1] == k, (a.shape, w.shape)
    if out is None:
        out = torch.empty(m, pad4(n), dtype=torch.float32, device=a.device)[:, :n]
    if m == 0 or n == 0:
        return out
    if bias is not None and (bias.requires_grad or bias.dtype != torch.float32 or not bias.is_contiguous()):
        bias = bias.detach().float().contiguous()
    if k == 0:      # nothing to multiply: the epilogue alone
        if bias is None:
            out.zero_()
        else:
            out.copy_(bias.expand(m, n))
        if addend is not None:
            out.add_(addend)
        return out.relu_() if relu else out
    with _span(tag):
        check(_lib.hip().lpf_gemm_f32(m, n, k, ptr(a), a.stride(0), ptr(w), w.stride(0), ptr(bias), ptr(addend),
                                      0 if addend is None else addend.stride(0), ptr(out), out.stride(0),
                                      FLAG_RELU if relu else 0, raw_stream(a.device)), "lpf_gemm_f32")
    return out


def layernorm_(x: torch.Tensor, g, b, relu=False, out=None, tag=None) -> torch.Tensor:
    """LayerNorm (eps 1e-5) (ReLU) of the rows of ``x`` through ``lpf_layernorm_f32``: in place, or into ``out``."""
    out = x if out is None else out
    with _span(tag):
        check(_lib.hip().lpf_layernorm_f32(x.shape[0], x.shape[1], ptr(x), x.stride(0), ptr(g), ptr(b), ptr(out),
                                           out.stride(0), FLAG_RELU if relu else 0, raw_stream(x.device)),
              "lpf_layernorm_f32")
    return out


def pair_gather(x: torch.Tensor, batch: torch.Tensor, *, product=None, sum=None, tag=None) -> None:
    """``product[m] = x[a_m] * x[b_m]`` and / or ``sum[m] = x[a_m] + x[b_m]`` for the pairs ``batch`` ([2, M] int64)
    through ``lpf_pair_gather_f32``: whichever of the two [M, D] outputs is given."""
    with _span(tag):
        check(_lib.hip().lpf_pair_gather_f32(batch.shape[1], x.shape[1], ptr(batch), batch.stride(0), x.shape[0], ptr(x),
                                             x.stride(0), ptr(product), 0 if product is None else product.stride(0),
                                             ptr(sum), 0 if sum is None else sum.stride(0), raw_stream(x.device)),
              "lpf_pair_gather_f32")


def long_rows(a, lo: int = 0, hi=None):
    """Hub rows (more than LPF_SPMM_LONG_ROW entries) of rows [lo, hi) of the ``DeviceCSR`` ``a``, as int32 row ids
    relative to ``lo``, or None when there is none; kept with the graph's ``Structure``, as long as that lives."""
    return a.structure.long_rows(lo, hi)


def spmm(a, t: torch.Tensor, lo: int = 0, hi=None, *, bias=None, ln=None, res=None, final_ln=None, relu=False,
         tag=None) -> torch.Tensor:
    """Rows [lo, hi) of ``a t`` through ``lpf_spmm_csr_f32`` / ``_bf16`` (by the dtype of ``t``), with the epilogue
    + bias -> LayerNorm ``ln`` -> ReLU -> + ``res`` -> LayerNorm ``final_ln`` (``ln`` / ``final_ln``: anything with
    ``weight`` and ``bias``); hub rows through the long-row kernel."""
    hi = a.n if hi is None else hi
    d = t.shape[1]
    rows = long_rows(a, lo, hi)
    out = torch.empty(hi - lo, d, dtype=torch.float32, device=t.device)
    name = "lpf_spmm_csr_bf16" if t.dtype == torch.bfloat16 else "lpf_spmm_csr_f32"
    with _span(tag):
        check(getattr(_lib.hip(), name)(
            hi - lo, d, ptr(a.rowptr) + 8 * lo, ptr(a.col), ptr(a.val), ptr(t), t.stride(0), ptr(out), out.stride(0),
            ptr(bias), ptr(ln.weight) if ln is not None else None, ptr(ln.bias) if ln is not None else None,
            ptr(res), 0 if res is None else res.stride(0),
            ptr(final_ln.weight) if final_ln is not None else None, ptr(final_ln.bias) if final_ln is not None else None,
            FLAG_RELU if relu else 0, ptr(rows), 0 if rows is None else rows.numel(), raw_stream(t.device)), name)
    return out
