"""torch.autograd.Function wrappers over the C ABI (include/rpde.h).

PyTorch is plumbing here: it owns device memory (outputs, tensors saved for
backward, workspaces all come from its caching allocator) and provides the
current HIP stream.  Every numerical step of the hot path runs in
librpde_hip.so.
"""
from __future__ import annotations

import contextlib
import os

import ctypes as C
from typing import Callable, List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import ACT, MODE, NORM, check, load, ptr, ptr_array, run, stream_ptr, workspace


def _f32c(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.float32:
        t = t.float()
    return t if t.is_contiguous() else t.contiguous()


def _as_float_storage(w: torch.Tensor) -> torch.Tensor:
    """complex64 [..] -> float32 [..,2] view of the same memory"""
    w = w if w.is_contiguous() else w.contiguous()
    return torch.view_as_real(w) if w.is_complex() else w


# ----------------------------------------------------------------------------
# frozen weights: evaluation loops (validation, all-resolution sweeps, rollouts -- reference train/training.py:78-123,
# utils/autoregressive_step.py) call the same layers hundreds of times with weights nobody touches.  Inside
# ``with frozen_weights():`` the no-grad paths of the FeedForward and of the 2-D spectral layer build their weight
# fragments (weight-norm / f16 pieces / mode-mix B operands) ONCE per layer and reuse them; the scope's end drops them.
# Contract: inside the scope the weights are changed, if at all, by torch in-place ops (which bump ``_version`` and
# refresh the entry) or by FlatAdamW.step, which writes through raw pointers and therefore calls
# ``invalidate_frozen()`` itself; any other raw-pointer writer must do the same.
# ----------------------------------------------------------------------------
_FROZEN: Optional[dict] = None


def invalidate_frozen() -> None:
    """drop every prepared buffer of the open scope (the scope itself stays open): for code that changes parameters
    without bumping ``_version`` -- FlatAdamW.step, a load through raw pointers"""
    if _FROZEN is not None:
        _FROZEN.clear()


@contextlib.contextmanager
def frozen_weights():
    global _FROZEN
    outer = _FROZEN
    if outer is None:
        _FROZEN = {}
    try:
        yield
    finally:
        if outer is None:
            _FROZEN = None


def _frozen_entry(kind, tensors, extra, nbytes, build, originals=None):
    """prepared buffer for these weight tensors, built by build(buf) on first use; None when no scope is open (or while
    a HIP graph is being captured: a graph must not hold a pointer whose life ends with the scope)"""
    if _FROZEN is None or torch.cuda.is_current_stream_capturing():
        return None
    # originals: what the caller was handed before _f32c.  Where _f32c had to copy (a parameter in another dtype or
    # layout) the copy has a new address on every call: caching by it would re-prepare every time and keep every copy
    # alive until the scope ends -- such weights take the unprepared path.
    if originals is not None and any(t is not o for t, o in zip(tensors, originals)):
        return None
    key = (kind, extra) + tuple(t.data_ptr() for t in tensors)
    ver = tuple(t._version for t in tensors)
    hit = _FROZEN.get(key)
    if hit is not None and hit[0] == ver:
        return hit[1]
    buf = hit[1] if hit is not None else torch.empty(nbytes, dtype=torch.uint8, device=tensors[0].device)
    build(buf)
    _FROZEN[key] = (ver, buf, tensors)          # (the tensors are held so that no data_ptr can be reused by another)
    return buf


# ----------------------------------------------------------------------------
# FSpectralConv{1,2}d.forward_fourier
# ----------------------------------------------------------------------------
class _FSpectral1d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, modes: int, mode: int, norm: int, with_skip: bool = False):
        lib = load()
        x = _f32c(x)
        wf = _f32c(w) if w is not None else None
        B, n, Cc = x.shape
        out = torch.empty_like(x)
        spec = torch.empty(lib.rpde_fspectral1d_spec_elems(B, n, Cc, modes), dtype=torch.float32, device=x.device)
        run("fspectral1d_fwd", lib.rpde_fspectral1d_ws_bytes(B, n, Cc, modes), x.device, ptr(x), ptr(wf), ptr(out),
            ptr(spec), B, n, Cc, modes, mode, norm)
        ctx.save_for_backward(spec, wf if wf is not None else x.new_empty(0))
        ctx.dims = (B, n, Cc, modes, mode, norm, wf is not None)
        # with_skip: also hand x back (an alias) for the caller's skip connection, so that the gradient
        # arriving through the skip is summed by the last backward GEMM's epilogue, not by a separate pass
        return (out, x.view_as(x)) if with_skip else out

    @staticmethod
    def backward(ctx, g, g_skip=None):
        lib = load()
        spec, wf = ctx.saved_tensors
        B, n, Cc, modes, mode, norm, has_w = ctx.dims
        if g is None:
            return g_skip, None, None, None, None, None
        g = _f32c(g)
        g_skip = _f32c(g_skip) if g_skip is not None else None
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1] and has_w
        gx = torch.empty_like(g) if need_x else None
        gw = torch.empty_like(wf) if need_w else None
        run("fspectral1d_bwd", lib.rpde_fspectral1d_ws_bytes(B, n, Cc, modes), g.device, ptr(g), ptr(spec),
            ptr(wf) if has_w else None, ptr(gx), ptr(gw), ptr(g_skip) if need_x else None, B, n, Cc, modes, mode, norm)
        return gx, gw, None, None, None, None


class _FSpectral2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, wy, wx, modes: int, mode: int, with_skip: bool = False):
        lib = load()
        x = _f32c(x)
        has_w = wy is not None
        wyf = _f32c(wy) if has_w else None
        wxf = _f32c(wx) if has_w else None
        B, M, N, Cc = x.shape
        out = torch.empty_like(x)
        spec_y = torch.empty(lib.rpde_fspectral2d_spec_elems(B, M, N, Cc, modes, 0), dtype=torch.float32, device=x.device)
        spec_x = torch.empty(lib.rpde_fspectral2d_spec_elems(B, M, N, Cc, modes, 1), dtype=torch.float32, device=x.device)
        run("fspectral2d_fwd", lib.rpde_fspectral2d_ws_bytes(B, M, N, Cc, modes), x.device, ptr(x), ptr(wyf),
            ptr(wxf), ptr(out), ptr(spec_y), ptr(spec_x), B, M, N, Cc, modes, mode)
        if has_w:
            ctx.save_for_backward(spec_y, spec_x, wyf, wxf)
        else:
            ctx.save_for_backward(spec_y, spec_x)
        ctx.dims = (B, M, N, Cc, modes, mode, has_w)
        return (out, x.view_as(x)) if with_skip else out

    @staticmethod
    def backward(ctx, g, g_skip=None):
        lib = load()
        B, M, N, Cc, modes, mode, has_w = ctx.dims
        if g is None:
            return g_skip, None, None, None, None, None
        if has_w:
            spec_y, spec_x, wyf, wxf = ctx.saved_tensors
        else:
            (spec_y, spec_x), wyf, wxf = ctx.saved_tensors, None, None
        g = _f32c(g)
        g_skip = _f32c(g_skip) if g_skip is not None else None
        need_x = ctx.needs_input_grad[0]
        need_w = has_w and (ctx.needs_input_grad[1] or ctx.needs_input_grad[2])
        gx = torch.empty_like(g) if need_x else None
        gwy = torch.empty_like(wyf) if need_w else None
        gwx = torch.empty_like(wxf) if need_w else None
        run("fspectral2d_bwd", lib.rpde_fspectral2d_ws_bytes(B, M, N, Cc, modes), g.device, ptr(g), ptr(spec_y),
            ptr(spec_x), ptr(wyf), ptr(wxf), ptr(gx), ptr(gwy), ptr(gwx), ptr(g_skip) if need_x else None, B, M, N,
            Cc, modes, mode)
        return gx, gwy, gwx, None, None, None


def _fspectral2d_frozen(x, wy, wx, modes: int):
    """evaluation inside frozen_weights(): rpde_fspectral2d_prepare once per layer, then rpde_fspectral2d_fwd_prepared
    (the spectra live in the workspace: nothing is kept for a backward).  None: this shape has nothing to prepare."""
    lib = load()
    x = _f32c(x)
    B, M, N, Cc = x.shape
    npre = lib.rpde_fspectral2d_prep_bytes(M, N, Cc, modes)
    if npre == 0:
        return None
    wyf, wxf = _f32c(wy), _f32c(wx)
    prep = _frozen_entry("fs2d", (wyf, wxf), (M, N, Cc, modes), npre, lambda buf: check(
        lib.rpde_fspectral2d_prepare(ptr(wyf), ptr(wxf), M, N, Cc, modes, buf.data_ptr(), npre, stream_ptr()),
        "fspectral2d_prepare"), originals=(wy, wx))
    if prep is None:
        return None
    out = torch.empty_like(x)
    run("fspectral2d_fwd_prepared", lib.rpde_fspectral2d_eval_ws_bytes(B, M, N, Cc, modes), x.device, ptr(x),
        prep.data_ptr(), ptr(out), B, M, N, Cc, modes)
    return out


def fspectral1d(x, w, modes: int, mode: str = "full", norm: str = "ortho", with_skip: bool = False):
    """FSpectralConv1d.forward_fourier: x [B,n,C], w [C,C,K,2].
    with_skip: returns (out, x') where x' aliases x -- use x' for a skip connection around the layer and
    its gradient is folded into the backward's last GEMM instead of a separate add."""
    if mode not in MODE:
        raise ValueError(f"Mode {mode} not recognized")
    return _FSpectral1d.apply(x, w if mode == "full" else None, int(modes), MODE[mode], NORM[norm], bool(with_skip))


def fspectral2d(x, wy, wx, modes: int, mode: str = "full", with_skip: bool = False):
    """FSpectralConv2d.forward_fourier: x [B,M,N,C], w_y/w_x [C,C,K,2].  with_skip: see fspectral1d."""
    if mode not in MODE:
        # the reference's 2-D layer has no else branch: both spectra stay zero
        return (torch.zeros_like(x), x) if with_skip else torch.zeros_like(x)
    full = mode == "full"
    if full and _FROZEN is not None and not torch.is_grad_enabled() and x.is_cuda:
        out = _fspectral2d_frozen(x, wy, wx, int(modes))
        if out is not None:
            return (out, x) if with_skip else out
    return _FSpectral2d.apply(x, wy if full else None, wx if full else None, int(modes), MODE[mode], bool(with_skip))


class _LiftedFSpectral2d(torch.autograd.Function):
    """forward_fourier(u W_in^T + b_in) from the thin u itself (csrc/lifted_spectral.hip): saves the spectra of u only
    and returns gradients for W_in, b_in and the two mode-mix weights -- none for u."""

    @staticmethod
    def forward(ctx, u, w_in, b_in, wy, wx, modes: int):
        lib = load()
        u, w_in, wyf, wxf = _f32c(u), _f32c(w_in), _f32c(wy), _f32c(wx)
        b_in = _f32c(b_in) if b_in is not None else None
        B, M, N, Cin = u.shape
        Cc = w_in.shape[0]
        out = torch.empty(B, M, N, Cc, dtype=torch.float32, device=u.device)
        spec = torch.empty(lib.rpde_lifted_fspectral2d_spec_elems(B, M, N, Cin, modes), dtype=torch.float32, device=u.device)
        run("lifted_fspectral2d_fwd", lib.rpde_fspectral2d_ws_bytes(B, M, N, Cc, modes), u.device, ptr(u), ptr(w_in),
            ptr(b_in), ptr(wyf), ptr(wxf), ptr(out), ptr(spec), B, M, N, Cc, Cin, modes)
        ctx.save_for_backward(spec, w_in, wyf, wxf, *(() if b_in is None else (b_in,)))
        ctx.dims = (B, M, N, Cc, Cin, modes)
        return out

    @staticmethod
    def backward(ctx, g):
        lib = load()
        B, M, N, Cc, Cin, modes = ctx.dims
        spec, w_in, wyf, wxf, *rest = ctx.saved_tensors
        b_in = rest[0] if rest else None
        g = _f32c(g)
        need_in, need_b = ctx.needs_input_grad[1], b_in is not None and ctx.needs_input_grad[2]
        need_w = ctx.needs_input_grad[3] or ctx.needs_input_grad[4]
        gw_in = torch.empty_like(w_in) if need_in else None
        gb_in = torch.empty_like(b_in) if need_b else None
        gwy = torch.empty_like(wyf) if need_w else None
        gwx = torch.empty_like(wxf) if need_w else None
        run("lifted_fspectral2d_bwd", lib.rpde_fspectral2d_ws_bytes(B, M, N, Cc, modes), g.device, ptr(g), ptr(spec),
            ptr(w_in), ptr(b_in), ptr(wyf), ptr(wxf), ptr(gw_in), ptr(gb_in), ptr(gwy), ptr(gwx), B, M, N, Cc, Cin, modes)
        return None, gw_in, gb_in, gwy, gwx, None


def lifted_fspectral2d_ok(u, w_in, modes: int) -> bool:
    """whether lifted_fspectral2d covers forward_fourier(linear(u, w_in, .)): a shape of the fused 2-D path, at most
    four input channels, fp32 on the GPU, and RPDE_LIFTED_SPECTRAL not 0.  Under no_grad the 64-channel path stays
    (fspectral2d): inside frozen_weights() its mode-mix fragments are built once per scope where W' would be rebuilt on
    every call, and evaluation is bit-identical with and without that scope"""
    if not (u.is_cuda and u.dim() == 4 and u.dtype == torch.float32 and w_in.dtype == torch.float32):
        return False
    if not torch.is_grad_enabled():
        return False
    _, M, N, Cin = u.shape
    return bool(load().rpde_lifted_fspectral2d_ok(M, N, w_in.shape[0], Cin, int(modes)))


def lifted_fspectral2d(u, w_in, b_in, wy, wx, modes: int):
    """FSpectralConv2d.forward_fourier (mode 'full') of h0 = linear(u, w_in, b_in), u [B,M,N,Cin <= 4] without a
    gradient of its own, w_in [C,Cin] the EFFECTIVE lifting weight: the lifting commutes with the DFT and folds into the
    mode-mix weights, so the spectral branch runs on Cin channels instead of C, and its backward needs neither an
    adjoint mix nor an adjoint synthesis (only weights receive gradients)."""
    return _LiftedFSpectral2d.apply(u, w_in, b_in, wy, wx, int(modes))


# ----------------------------------------------------------------------------
# dropout masks under a captured hipGraph: a replay repeats its launch arguments, so the seed the FeedForward draws on
# the host would freeze one mask for ever.  Every dropout kernel therefore also mixes a DEVICE counter into its seed
# (rpde_ff_params.seed_epoch); eager steps leave it at 0 (the host seed changes per call), a GraphedTrainStep advances it
# once per replay -- on the device, inside the graph -- before the forward, so forward and backward of one step agree.
# ----------------------------------------------------------------------------
_DROP_EPOCH: dict = {}


def drop_epoch(device) -> torch.Tensor:
    """the int64 [1] device counter of `device` (created on first use, 0)"""
    dev = torch.device(device)
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    t = _DROP_EPOCH.get(key)
    if t is None:
        t = torch.zeros(1, dtype=torch.int64, device=dev)
        _DROP_EPOCH[key] = t
    return t


# ----------------------------------------------------------------------------
# FeedForward (+ residual / post-activation glue)
# ----------------------------------------------------------------------------
class _FeedForward(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, residual, cfg, *params):
        """cfg = (n_layers, dim, factor, layer_norm, eps, dropout_p, seed, post_act)
        params = W0, b0, ..., W_{L-1}, b_{L-1} [, gamma, beta]"""
        lib = load()
        L, dim, factor, layer_norm, eps, p_drop, seed, post_act, grad_on = cfg
        shape = x.shape
        x2 = _f32c(x).reshape(-1, dim)
        P = x2.shape[0]
        res2 = _f32c(residual).reshape(-1, dim) if residual is not None else None
        ws_ = [_f32c(params[2 * l]) for l in range(L)]
        bs_ = [_f32c(params[2 * l + 1]) for l in range(L)]
        gamma = _f32c(params[2 * L]) if layer_norm else None
        beta = _f32c(params[2 * L + 1]) if layer_norm else None
        need_grad = grad_on and any(ctx.needs_input_grad)     # (grad mode is always off inside forward itself)
        hid = dim * factor
        # the fused kernel keeps the hidden activations on chip: in evaluation nothing but `out` is allocated
        # (the fused kernels' weight preparation reads 16 bytes at a time: a weight view at an odd storage offset takes the
        #  per-GEMM path inside the library, which needs the hidden buffers -- so it must not be "lean" here either)
        fused = bool(lib.rpde_feedforward_is_fused(dim, factor, L, P)) and all(w.data_ptr() % 16 == 0 for w in ws_)
        lean = (not need_grad) and fused
        # RPDE_FF_STASH=u: training through the fused kernels saves only u = dropout(z) of the hidden layers (in `hs`) and
        # the backward kernels re-evaluate gelu / gelu' from it -- half the saved-for-backward footprint, but measured
        # slower on MI355X (the erf-class vector work costs more than the 2 KB per point it keeps out of HBM:
        # DESIGN.md section 6).  Default: h and d = gelu'(u) * dropscale are stored once by the forward kernel.
        recompute = need_grad and fused and os.environ.get("RPDE_FF_STASH", "hd") == "u"
        hs = [None if lean else torch.empty(P, hid, dtype=torch.float32, device=x.device) for _ in range(L - 1)]
        ds = [torch.empty(P, hid, dtype=torch.float32, device=x.device) if (need_grad and not recompute) else None
              for _ in range(L - 1)]
        out = torch.empty(P, dim, dtype=torch.float32, device=x.device)
        # (the pre-LayerNorm tensor is saved for backward only: the evaluation kernel does not write it)
        z_last = out if lean else torch.empty(P, dim, dtype=torch.float32, device=x.device)
        wa, ba, ha, da = ptr_array(ws_), ptr_array(bs_), ptr_array(hs or [None]), ptr_array(ds or [None])
        epoch = drop_epoch(x.device).data_ptr() if p_drop > 0.0 else None
        fp = _lib.FFParams(L, dim, factor, int(layer_norm), eps, p_drop, seed, post_act,
                           C.cast(wa, C.POINTER(C.c_void_p)), C.cast(ba, C.POINTER(C.c_void_p)), ptr(gamma), ptr(beta), epoch)
        nws = lib.rpde_feedforward_fwd_ws_bytes(dim, factor, L)
        if lean and p_drop == 0.0:
            held = tuple(ws_ + bs_ + ([gamma, beta] if layer_norm else []))
            orig = tuple([params[2 * l] for l in range(L)] + [params[2 * l + 1] for l in range(L)] +
                         ([params[2 * L], params[2 * L + 1]] if layer_norm else []))
            prep = _frozen_entry("ff", held, (L, dim, factor), nws, lambda buf: check(
                lib.rpde_feedforward_prepare(C.byref(fp), buf.data_ptr(), nws, stream_ptr()), "feedforward_prepare"),
                originals=orig)
            if prep is not None:
                check(lib.rpde_feedforward_fwd_prepared(C.byref(fp), ptr(x2), ptr(res2), ptr(out), P, prep.data_ptr(), nws,
                                                        stream_ptr()), "feedforward_fwd_prepared")
                return out.reshape(shape)
        run("feedforward_fwd", nws, x.device, C.byref(fp), ptr(x2), ptr(res2), C.cast(ha, C.POINTER(C.c_void_p)),
            C.cast(da, C.POINTER(C.c_void_p)), ptr(z_last), ptr(out), P)
        ctx.cfg = cfg
        ctx.has_res = residual is not None
        if need_grad:
            ctx.save_for_backward(x2, z_last, *hs, *ds, *ws_, *bs_, *([gamma, beta] if layer_norm else []))
        return out.reshape(shape)

    @staticmethod
    def backward(ctx, g):
        lib = load()
        L, dim, factor, layer_norm, eps, p_drop, seed, post_act, _ = ctx.cfg
        saved = ctx.saved_tensors
        x2, z_last = saved[0], saved[1]
        o = 2
        hs, ds = list(saved[o:o + L - 1]), list(saved[o + L - 1:o + 2 * (L - 1)])
        o += 2 * (L - 1)
        ws_, bs_ = list(saved[o:o + L]), list(saved[o + L:o + 2 * L])
        gamma, beta = (saved[o + 2 * L], saved[o + 2 * L + 1]) if layer_norm else (None, None)
        P = x2.shape[0]
        g2 = _f32c(g).reshape(-1, dim)
        gx = torch.empty_like(x2) if ctx.needs_input_grad[0] else None
        gws = [torch.empty_like(w) for w in ws_]
        gbs = [torch.empty_like(b) for b in bs_]
        ggamma = torch.empty_like(gamma) if layer_norm else None
        gbeta = torch.empty_like(beta) if layer_norm else None
        wa, ba, ha, da = ptr_array(ws_), ptr_array(bs_), ptr_array(hs or [None]), ptr_array(ds or [None])
        gwa, gba = ptr_array(gws), ptr_array(gbs)
        epoch = drop_epoch(g.device).data_ptr() if p_drop > 0.0 else None
        fp = _lib.FFParams(L, dim, factor, int(layer_norm), eps, p_drop, seed, post_act,
                           C.cast(wa, C.POINTER(C.c_void_p)), C.cast(ba, C.POINTER(C.c_void_p)), ptr(gamma), ptr(beta), epoch)
        run("feedforward_bwd", lib.rpde_feedforward_ws_bytes(P, dim, factor, L), g.device, C.byref(fp), ptr(x2),
            C.cast(ha, C.POINTER(C.c_void_p)), C.cast(da, C.POINTER(C.c_void_p)), ptr(z_last), ptr(g2), ptr(gx),
            C.cast(gwa, C.POINTER(C.c_void_p)), C.cast(gba, C.POINTER(C.c_void_p)), ptr(ggamma), ptr(gbeta), P)
        grads: List[Optional[torch.Tensor]] = []
        for l in range(L):
            grads += [gws[l], gbs[l]]
        if layer_norm:
            grads += [ggamma, gbeta]
        gres = g if ctx.has_res else None
        return (gx.reshape(g.shape) if gx is not None else None, gres, None, *grads)


def feedforward(x, residual, weights: Sequence[torch.Tensor], biases: Sequence[torch.Tensor], ln: Optional[Tuple],
                dim: int, factor: int, dropout_p: float, seed: int, post_act: str = "identity", eps: float = 1e-5):
    L = len(weights)
    params: List[torch.Tensor] = []
    for w, b in zip(weights, biases):
        params += [w, b]
    if ln is not None:
        params += [ln[0], ln[1]]
    cfg = (L, int(dim), int(factor), ln is not None, float(eps), float(dropout_p), int(seed) & (2 ** 64 - 1), ACT[post_act],
           torch.is_grad_enabled())
    return _FeedForward.apply(x, residual, cfg, *params)


# ----------------------------------------------------------------------------
# pointwise linear (channels-last)
# ----------------------------------------------------------------------------
class _Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        lib = load()
        in_f, out_f = w.shape[1], w.shape[0]
        x2 = _f32c(x).reshape(-1, in_f)
        w = _f32c(w)
        b = _f32c(b) if b is not None else None
        P = x2.shape[0]
        out = torch.empty(P, out_f, dtype=torch.float32, device=x.device)
        check(lib.rpde_linear_fwd(ptr(x2), ptr(w), ptr(b), ptr(out), P, in_f, out_f, stream_ptr()), "linear_fwd")
        ctx.save_for_backward(x2, w)
        ctx.has_b = b is not None
        return out.reshape(*x.shape[:-1], out_f)

    @staticmethod
    def backward(ctx, g):
        lib = load()
        x2, w = ctx.saved_tensors
        out_f, in_f = w.shape
        P = x2.shape[0]
        g2 = _f32c(g).reshape(-1, out_f)
        gx = torch.empty_like(x2) if ctx.needs_input_grad[0] else None
        gw = torch.empty_like(w) if ctx.needs_input_grad[1] else None
        gb = torch.empty(out_f, dtype=torch.float32, device=g.device) if (ctx.has_b and ctx.needs_input_grad[2]) else None
        run("linear_bwd", lib.rpde_linear_ws_bytes(P, in_f, out_f), g.device, ptr(x2), ptr(w), ptr(g2), ptr(gx),
            ptr(gw), ptr(gb), P, in_f, out_f)
        return (gx.reshape(*g.shape[:-1], in_f) if gx is not None else None), gw, gb


def linear(x, w, b=None):
    return _Linear.apply(x, w, b)


class _WeightNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v, g):
        lib = load()
        v = _f32c(v)
        g = _f32c(g)
        out_f, in_f = v.shape
        w = torch.empty_like(v)
        check(lib.rpde_weight_norm_fwd(ptr(v), ptr(g), ptr(w), out_f, in_f, stream_ptr()), "weight_norm_fwd")
        ctx.save_for_backward(v, g)
        return w

    @staticmethod
    def backward(ctx, gw):
        lib = load()
        v, g = ctx.saved_tensors
        out_f, in_f = v.shape
        gw = _f32c(gw)
        gv = torch.empty_like(v) if ctx.needs_input_grad[0] else None
        gg = torch.empty_like(g) if ctx.needs_input_grad[1] else None
        if gv is None and gg is None:
            return None, None
        check(lib.rpde_weight_norm_bwd(ptr(v), ptr(g), ptr(gw), ptr(gv), ptr(gg), out_f, in_f, stream_ptr()), "weight_norm_bwd")
        return gv, gg


def weight_norm(v, g):
    """WNLinear's effective weight v * (g / |v|_row) (models/custom_layer.py:70-108), v [out,in], g [out,1]"""
    return _WeightNorm.apply(v, g)


# ----------------------------------------------------------------------------
# FNO: channels-first spectral conv, 1x1 conv, activation
# ----------------------------------------------------------------------------
class _Spectral1d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, act_in: int):
        lib = load()
        x = _f32c(x)
        wf = _as_float_storage(w)
        B, Ci, n = x.shape
        Co, K = w.shape[1], w.shape[2]
        out = torch.empty(B, Co, n, dtype=torch.float32, device=x.device)
        kp = (K + 3) // 4 * 4
        spec = torch.empty(B * Ci * 2 * kp, dtype=torch.float32, device=x.device)
        run("spectral1d_fwd", lib.rpde_spectral1d_ws_bytes(B, Ci, Co, n, K), x.device, ptr(x), ptr(wf), ptr(out),
            ptr(spec), B, Ci, Co, n, K, act_in)
        ctx.save_for_backward(spec, w, x if act_in else x.new_empty(0))
        ctx.dims = (B, Ci, Co, n, K, act_in)
        return out

    @staticmethod
    def backward(ctx, g):
        lib = load()
        spec, w, x = ctx.saved_tensors
        B, Ci, Co, n, K, act_in = ctx.dims
        g = _f32c(g)
        wf = _as_float_storage(w)
        gx = torch.empty(B, Ci, n, dtype=torch.float32, device=g.device) if ctx.needs_input_grad[0] else None
        gw = torch.empty_like(w) if ctx.needs_input_grad[1] else None
        run("spectral1d_bwd", lib.rpde_spectral1d_ws_bytes(B, Ci, Co, n, K), g.device, ptr(g), ptr(spec), ptr(wf),
            ptr(x) if act_in else None, ptr(gx), ptr(_as_float_storage(gw)) if gw is not None else None, B, Ci, Co, n,
            K, act_in)
        return gx, gw, None


class _Spectral2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w1, w2, act_in: int):
        lib = load()
        x = _f32c(x)
        B, Ci, M, N = x.shape
        Co, m1, m2 = w1.shape[1], w1.shape[2], w1.shape[3]
        out = torch.empty(B, Co, M, N, dtype=torch.float32, device=x.device)
        spec = torch.empty(lib.rpde_spectral2d_spec_elems(B, Ci, M, N, m1, m2), dtype=torch.float32, device=x.device)
        run("spectral2d_fwd", lib.rpde_spectral2d_ws_bytes(B, Ci, Co, M, N, m1, m2), x.device, ptr(x),
            ptr(_as_float_storage(w1)), ptr(_as_float_storage(w2)), ptr(out), ptr(spec), B, Ci, Co, M, N, m1, m2,
            act_in)
        ctx.save_for_backward(spec, w1, w2, x if act_in else x.new_empty(0))
        ctx.dims = (B, Ci, Co, M, N, m1, m2, act_in)
        return out

    @staticmethod
    def backward(ctx, g):
        lib = load()
        spec, w1, w2, x = ctx.saved_tensors
        B, Ci, Co, M, N, m1, m2, act_in = ctx.dims
        g = _f32c(g)
        gx = torch.empty(B, Ci, M, N, dtype=torch.float32, device=g.device) if ctx.needs_input_grad[0] else None
        need_w = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        gw1 = torch.empty_like(w1) if need_w else None
        gw2 = torch.empty_like(w2) if need_w else None
        run("spectral2d_bwd", lib.rpde_spectral2d_ws_bytes(B, Ci, Co, M, N, m1, m2), g.device, ptr(g), ptr(spec),
            ptr(_as_float_storage(w1)), ptr(_as_float_storage(w2)), ptr(x) if act_in else None, ptr(gx),
            ptr(_as_float_storage(gw1)) if need_w else None, ptr(_as_float_storage(gw2)) if need_w else None, B, Ci,
            Co, M, N, m1, m2, act_in)
        return gx, gw1, gw2, None


def spectral1d(x, w, act_in: str = "identity"):
    if w.shape[2] > x.shape[-1] // 2 + 1:
        raise RuntimeError(f"SpectralConv1d: modes1={w.shape[2]} exceeds n//2+1={x.shape[-1] // 2 + 1}")
    return _Spectral1d.apply(x, w, ACT[act_in])


def spectral2d(x, w1, w2, act_in: str = "identity"):
    if w1.shape[3] > x.shape[-1] // 2 + 1 or w1.shape[2] > x.shape[-2]:
        raise RuntimeError("SpectralConv2d: modes exceed the available spectrum")
    return _Spectral2d.apply(x, w1, w2, ACT[act_in])


class _Conv1x1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, act_in: int, acc, acc_owned: bool = False):
        """out = (acc +) W . act(x) + b ; x [B,Cin,*S] channels-first, w [Cout,Cin,1(,1)]
        acc_owned: the caller hands over `acc` (a temporary it will not read again): accumulate in place even
        when autograd cannot tell (no_grad / eval, where every tensor is a leaf)"""
        lib = load()
        x = _f32c(x)
        B, Ci = x.shape[0], x.shape[1]
        S = x[0, 0].numel()
        Co = w.shape[0]
        w2 = _f32c(w).reshape(Co, Ci)
        b = _f32c(b) if b is not None else None
        if acc is not None:
            if acc.dtype == torch.float32 and acc.is_contiguous() and (not acc.is_leaf or (acc_owned and not acc.requires_grad)):
                ctx.mark_dirty(acc)          # accumulate in place into the spectral branch's output
                out = acc
            else:
                out = _f32c(acc).clone()
        else:
            out = torch.empty(B, Co, *x.shape[2:], dtype=torch.float32, device=x.device)
        check(lib.rpde_conv1x1_fwd(ptr(x), ptr(w2), ptr(b), ptr(out), B, Ci, Co, S, act_in, int(acc is not None),
                                   stream_ptr()), "conv1x1_fwd")
        ctx.save_for_backward(x, w2)
        ctx.meta = (B, Ci, Co, S, act_in, b is not None, acc is not None, w.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        lib = load()
        x, w2 = ctx.saved_tensors
        B, Ci, Co, S, act_in, has_b, has_acc, wshape = ctx.meta
        g = _f32c(g)
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        gw = torch.empty_like(w2) if ctx.needs_input_grad[1] else None
        gb = torch.empty(Co, dtype=torch.float32, device=g.device) if (has_b and ctx.needs_input_grad[2]) else None
        run("conv1x1_bwd", lib.rpde_conv1x1_ws_bytes(B, Ci, Co, S), g.device, ptr(x), ptr(w2), ptr(g), ptr(gx),
            ptr(gw), ptr(gb), B, Ci, Co, S, act_in, 0)
        return gx, (gw.reshape(wshape) if gw is not None else None), gb, None, (g if has_acc else None), None


def conv1x1(x, w, b=None, act_in: str = "identity", acc=None, acc_owned: bool = False):
    return _Conv1x1.apply(x, w, b, ACT[act_in], acc, acc_owned)


def conv1x1_act_eval(x, w, b, acc, act_out: str):
    """evaluation only (no autograd): acc <- act_out(acc + W . x + b), in place in the temporary `acc`"""
    lib = load()
    x = _f32c(x)
    B, Ci = x.shape[0], x.shape[1]
    S = x[0, 0].numel()
    Co = w.shape[0]
    w2 = _f32c(w.detach()).reshape(Co, Ci)
    bb = _f32c(b.detach()) if b is not None else None
    out = acc if (acc.dtype == torch.float32 and acc.is_contiguous()) else _f32c(acc).clone()
    check(lib.rpde_conv1x1_act_fwd(ptr(x), ptr(w2), ptr(bb), ptr(out), B, Ci, Co, S, 0, 1, ACT[act_out], stream_ptr()),
          "conv1x1_act_fwd")
    return out


def fnoblock2d_eval(x, w1, w2, wc, bc, act_out: str):
    """evaluation only (no autograd): act_out(SpectralConv2d(x; w1, w2) + conv1x1(x; wc, bc)) with the spectral branch's
    last transform, the bypass convolution and the activation in one pass over x; None when the shape is not covered"""
    lib = load()
    if x.dim() != 4 or w1.shape[3] > x.shape[-1] // 2 + 1 or w1.shape[2] > x.shape[-2]:
        return None
    B, Ci, M, N = x.shape
    Co, m1, m2 = w1.shape[1], w1.shape[2], w1.shape[3]
    if not lib.rpde_fnoblock2d_eval_ok(Ci, Co, M, N, m2):
        return None
    x = _f32c(x)
    wcf = _f32c(wc.detach()).reshape(Co, Ci)
    bcf = _f32c(bc.detach()) if bc is not None else None
    out = torch.empty(B, Co, M, N, dtype=torch.float32, device=x.device)
    run("fnoblock2d_eval_fwd", lib.rpde_fnoblock2d_eval_ws_bytes(B, Ci, Co, M, N, m1, m2), x.device, ptr(x),
        ptr(_as_float_storage(w1.detach())), ptr(_as_float_storage(w2.detach())), ptr(wcf), ptr(bcf), ptr(out), B, Ci,
        Co, M, N, m1, m2, ACT[act_out])
    return out


def fnoblock2d_proj_eval(x, w1, w2, wc, bc, act_out: str, pw1, pb1, pw2, pb2):
    """evaluation only (no autograd): the LAST FNO block and the projection MLP in one library call --
    mlp2(gelu(mlp1(act_out(SpectralConv2d(x; w1, w2) + conv1x1(x; wc, bc))))) -- without the block's output ever being
    written (rpde_fnoblock2d_proj_eval_fwd); None when the shape is not covered"""
    lib = load()
    if x.dim() != 4 or not x.is_cuda or w1.shape[3] > x.shape[-1] // 2 + 1 or w1.shape[2] > x.shape[-2]:
        return None
    B, Ci, M, N = x.shape
    Co, m1, m2 = w1.shape[1], w1.shape[2], w1.shape[3]
    Cm, Cq = pw1.shape[0], pw2.shape[0]
    if pw1[0].numel() != Co or pw2[0].numel() != Cm or not lib.rpde_fnoblock2d_proj_eval_ok(Ci, Co, M, N, m1, m2, Cm, Cq):
        return None
    x = _f32c(x)
    wcf = _f32c(wc.detach()).reshape(Co, Ci)
    bcf = _f32c(bc.detach()) if bc is not None else None
    p1, p2 = _f32c(pw1.detach()).reshape(Cm, Co), _f32c(pw2.detach()).reshape(Cq, Cm)
    q1 = _f32c(pb1.detach()) if pb1 is not None else None
    q2 = _f32c(pb2.detach()) if pb2 is not None else None
    out = torch.empty(B, Cq, M, N, dtype=torch.float32, device=x.device)
    run("fnoblock2d_proj_eval_fwd", lib.rpde_fnoblock2d_eval_ws_bytes(B, Ci, Co, M, N, m1, m2), x.device, ptr(x),
        ptr(_as_float_storage(w1.detach())), ptr(_as_float_storage(w2.detach())), ptr(wcf), ptr(bcf), ptr(p1),
        ptr(q1), ptr(p2), ptr(q2), ptr(out), B, Ci, Co, M, N, m1, m2, ACT[act_out], Cm, Cq)
    return out


def fno2d_lift_block_eval(u, gx, gy, wl, bl, w1, w2, wc, bc, act_out: str):
    """evaluation only (no autograd): act_out(SpectralConv2d(x0) + conv1x1(x0)) with x0 = lifting(cat(u, gx, gy)) formed on
    the fly (rpde_fno2d_lift_block_eval_fwd: the lifted field is never written); u [B,1,M,N], gx [M], gy [N] device
    arrays.  None when the shape is not covered."""
    lib = load()
    if u.dim() != 4 or u.shape[1] != 1 or not u.is_cuda:
        return None
    B, _, M, N = u.shape
    C, Co, m1, m2 = w1.shape[0], w1.shape[1], w1.shape[2], w1.shape[3]
    if wl.shape[0] != C or wl[0].numel() != 3 or not lib.rpde_fno2d_lift_block_eval_ok(1, C, Co, M, N, m1, m2):
        return None
    u = _f32c(u)
    gx, gy = _f32c(gx), _f32c(gy)
    wlf = _f32c(wl.detach()).reshape(C, 3)
    blf = _f32c(bl.detach()) if bl is not None else None
    wcf = _f32c(wc.detach()).reshape(Co, C)
    bcf = _f32c(bc.detach()) if bc is not None else None
    out = torch.empty(B, Co, M, N, dtype=torch.float32, device=u.device)
    run("fno2d_lift_block_eval_fwd", lib.rpde_fno2d_lift_block_eval_ws_bytes(B, C, Co, M, N, m1, m2), u.device,
        ptr(u), ptr(gx), ptr(gy), ptr(wlf), ptr(blf), ptr(_as_float_storage(w1.detach())),
        ptr(_as_float_storage(w2.detach())), ptr(wcf), ptr(bcf), ptr(out), B, C, Co, M, N, m1, m2, ACT[act_out])
    return out


def conv_mlp_eval(x, w1, b1, w2, b2, act_in: str = "identity"):
    """evaluation only (no autograd): mlp2(gelu(mlp1(act_in(x)))) of the FNO projection in one pass, or None when the
    shape is not covered (the caller then runs the two convolutions)"""
    lib = load()
    B, Ci = x.shape[0], x.shape[1]
    S = x[0, 0].numel()
    Cm, Co = w1.shape[0], w2.shape[0]
    if not lib.rpde_conv_mlp_ok(Ci, Cm, Co, S):
        return None
    x = _f32c(x)
    w1f, w2f = _f32c(w1.detach()).reshape(Cm, Ci), _f32c(w2.detach()).reshape(Co, Cm)
    b1f = _f32c(b1.detach()) if b1 is not None else None
    b2f = _f32c(b2.detach()) if b2 is not None else None
    out = torch.empty(B, Co, *x.shape[2:], dtype=torch.float32, device=x.device)
    check(lib.rpde_conv_mlp_fwd(ptr(x), ptr(w1f), ptr(b1f), ptr(w2f), ptr(b2f), ptr(out), B, Ci, Cm, Co, S, ACT[act_in],
                                stream_ptr()), "conv_mlp_fwd")
    return out


class _Act(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, act: int):
        lib = load()
        x = _f32c(x)
        out = torch.empty_like(x)
        check(lib.rpde_act_fwd(ptr(x), ptr(out), x.numel(), act, stream_ptr()), "act_fwd")
        ctx.save_for_backward(x)
        ctx.act = act
        return out

    @staticmethod
    def backward(ctx, g):
        lib = load()
        (x,) = ctx.saved_tensors
        g = _f32c(g)
        dx = torch.empty_like(x)
        check(lib.rpde_act_bwd(ptr(x), ptr(g), ptr(dx), x.numel(), ctx.act, stream_ptr()), "act_bwd")
        return dx, None


def activation(x, act: str):
    return x if act == "identity" else _Act.apply(x, ACT[act])


# ----------------------------------------------------------------------------
# model-boundary layout helpers
# ----------------------------------------------------------------------------
class _ConcatGrid(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, grid_dims: int, lo: float, hi: float, channels_last: bool, gx, gy):
        lib = load()
        x = _f32c(x)
        B, Ci = x.shape[0], x.shape[1]
        sp = tuple(x.shape[2:])
        M, N = (sp[0], 1) if len(sp) == 1 else sp
        Ct = Ci + grid_dims
        shape = (B, *sp, Ct) if channels_last else (B, Ct, *sp)
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
        check(lib.rpde_concat_grid(ptr(x), ptr(out), B, Ci, M, N, grid_dims, lo, hi, int(channels_last),
                                   ptr(gx), ptr(gy), stream_ptr()), "concat_grid")
        ctx.meta = (Ci, channels_last, len(sp))
        return out

    @staticmethod
    def backward(ctx, g):
        Ci, channels_last, nd = ctx.meta
        if channels_last:
            gx = g[..., :Ci]
            gx = gx.permute(0, nd + 1, *range(1, nd + 1))
        else:
            gx = g[:, :Ci]
        return gx.contiguous(), None, None, None, None, None, None


def concat_grid(x, grid_dims: int, lo: float = 0.0, hi: float = 1.0, channels_last: bool = True, gridx=None, gridy=None):
    return _ConcatGrid.apply(x, grid_dims, float(lo), float(hi), bool(channels_last), gridx, gridy)


class _TransposeCS(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, to_channels_first: bool):
        """to_channels_first: [B,*S,C] -> [B,C,*S];  else the inverse"""
        lib = load()
        x = _f32c(x)
        B = x.shape[0]
        if to_channels_first:
            sp, Cc = tuple(x.shape[1:-1]), x.shape[-1]
            out = torch.empty(B, Cc, *sp, dtype=torch.float32, device=x.device)
        else:
            Cc, sp = x.shape[1], tuple(x.shape[2:])
            out = torch.empty(B, *sp, Cc, dtype=torch.float32, device=x.device)
        S = 1
        for s in sp:
            S *= s
        check(lib.rpde_transpose_cs(ptr(x), ptr(out), B, S, Cc, int(to_channels_first), stream_ptr()), "transpose_cs")
        ctx.tcf = to_channels_first
        return out

    @staticmethod
    def backward(ctx, g):
        return _TransposeCS.apply(g, not ctx.tcf), None


def to_channels_first(x):
    if x.shape[-1] == 1:
        return x.reshape(x.shape[0], 1, *x.shape[1:-1])
    return _TransposeCS.apply(x, True)


def to_channels_last(x):
    if x.shape[1] == 1:
        return x.reshape(x.shape[0], *x.shape[2:], 1)
    return _TransposeCS.apply(x, False)


# ----------------------------------------------------------------------------
# relative L2 loss; the three helpers serve the whole family (csrc/rel_loss.hip)
# ----------------------------------------------------------------------------
def _rel_outputs(B: int, device, reduction: bool, stats_elems: Optional[int] = None):
    """(stats, rel, loss or None) of a relative loss: stats [2 B] unless the entry asks for more"""
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=device)          # noqa: E731
    return new(stats_elems or 2 * B), new(B), new() if reduction else None


def _upstream(g: torch.Tensor, reduction: bool):
    """(grad_loss, grad_rel) for an entry's backward: the scalar's gradient, or the per-sample vector's"""
    return (ptr(g), None) if reduction else (None, ptr(g))


def _bcmn(x: torch.Tensor, dims: int):
    """(B, C, M, N) of a channels-first field, M = 1 for dims = 1"""
    return (x.shape[0], x.shape[1], 1, x.shape[2]) if dims == 1 else tuple(x.shape[:4])


class _RelL2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, size_average: bool, reduction: bool):
        lib = load()
        x = _f32c(x)
        y = _f32c(y)
        B = x.shape[0]
        per = x.numel() // B
        if y.numel() != x.numel():
            raise RuntimeError(f"RelativeL2Loss: shapes {tuple(x.shape)} and {tuple(y.shape)} differ in size")
        stats, rel, loss = _rel_outputs(B, x.device, reduction, lib.rpde_rel_l2_stats_elems(B))
        check(lib.rpde_rel_l2_fwd(ptr(x), ptr(y), ptr(rel), ptr(loss), ptr(stats), B, per, int(size_average),
                                  stream_ptr()), "rel_l2_fwd")
        ctx.save_for_backward(x, y, stats)
        ctx.meta = (B, per, size_average, reduction)
        return loss if reduction else rel

    @staticmethod
    def backward(ctx, g):
        lib = load()
        x, y, stats = ctx.saved_tensors
        B, per, size_average, reduction = ctx.meta
        g = _f32c(g)
        gx = torch.empty_like(x)
        check(lib.rpde_rel_l2_bwd(ptr(x), ptr(y), ptr(stats), *_upstream(g, reduction), ptr(gx), B, per, int(size_average),
                                  stream_ptr()), "rel_l2_bwd")
        return gx, None, None, None


def relative_l2(x, y, size_average: bool = True, reduction: bool = True):
    return _RelL2.apply(x, y, bool(size_average), bool(reduction))


# ----------------------------------------------------------------------------
# mode-weighted relative L2 loss (csrc/spectral_loss.hip, rpde_wrel_l2_*; utils/loss.py SpectralRelativeL2Loss)
# ----------------------------------------------------------------------------
class _WRelL2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, omega, dims: int, size_average: bool, reduction: bool):
        lib = load()
        if x.dim() != dims + 2 or x.shape != y.shape:
            raise ValueError(f"weighted_relative_l2: x {tuple(x.shape)} / y {tuple(y.shape)}, expected equal "
                             f"{dims + 2}-D channels-first shapes")
        B, Cc, M, N = _bcmn(x, dims)
        want = (N // 2 + 1,) if dims == 1 else (M, N // 2 + 1)
        if tuple(omega.shape) != want:
            raise ValueError(f"weighted_relative_l2: omega {tuple(omega.shape)}, expected {want} for the grid {tuple(x.shape[2:])}")
        x, y = _f32c(x), _f32c(y)
        px, py, pw = ptr(x), ptr(y), ptr(omega)               # raises for CPU tensors: there is no fallback
        stats, rel, loss = _rel_outputs(B, x.device, reduction)
        spec = torch.empty(lib.rpde_wrel_l2_spec_elems(B, Cc, M, N), dtype=torch.float32, device=x.device)
        run("wrel_l2_fwd", lib.rpde_wrel_l2_ws_bytes(B, Cc, M, N), x.device, px, py, pw, ptr(rel), ptr(loss),
            ptr(stats), ptr(spec), B, Cc, M, N, int(size_average))
        ctx.save_for_backward(spec, omega, stats)
        ctx.meta = (tuple(x.shape), B, Cc, M, N, size_average, reduction)
        return loss if reduction else rel

    @staticmethod
    def backward(ctx, g):
        lib = load()
        spec, omega, stats = ctx.saved_tensors
        shape, B, Cc, M, N, size_average, reduction = ctx.meta
        g = _f32c(g)
        gx = torch.empty(shape, dtype=torch.float32, device=spec.device)
        run("wrel_l2_bwd", lib.rpde_wrel_l2_ws_bytes(B, Cc, M, N), spec.device, ptr(spec), ptr(omega), ptr(stats),
            *_upstream(g, reduction), ptr(gx), B, Cc, M, N, int(size_average))
        return gx, None, None, None, None, None


def weighted_relative_l2(x, y, omega, dims: int, size_average: bool = True, reduction: bool = True):
    """rel[b] = sqrt(E(x - y)[b]) / (sqrt(E(y)[b]) + 1e-8), E(z)[b] = sum_c sum_k omega_k c_kx / N |rfft(z)[b,c,k]|^2, then
    mean / sum / the per-sample vector as relative_l2.  x, y [B, C, n] (dims=1) or [B, C, H, W] (dims=2) and omega
    [n//2+1] / [H, W//2+1] (>= 0, rows in fft order; validated by utils.loss.SpectralRelativeL2Loss) are contiguous
    fp32 tensors on the GPU.  Gradient for x only."""
    if dims not in (1, 2):
        raise ValueError(f"weighted_relative_l2: dims must be 1 or 2, got {dims}")
    return _WRelL2.apply(x, y, omega, int(dims), bool(size_average), bool(reduction))


# ----------------------------------------------------------------------------
# spectral resize (csrc/resize.hip; evaluation-time data path, no autograd)
# ----------------------------------------------------------------------------
def resize1d(x: torch.Tensor, out_size: int) -> torch.Tensor:
    """x [..., n] -> [..., out_size]: rfft, keep the shared bins, irfft(out_size), times out/in"""
    lib = load()
    x = _f32c(x.detach())
    n = x.shape[-1]
    rows = x.numel() // n
    out = torch.empty(*x.shape[:-1], int(out_size), dtype=torch.float32, device=x.device)
    run("resize1d", lib.rpde_resize1d_ws_bytes(rows, n, int(out_size)), x.device, ptr(x), ptr(out), rows, n,
        int(out_size))
    return out


def resize2d(x: torch.Tensor, out_size) -> torch.Tensor:
    """x [..., M, N] -> [..., Mo, No] (reference utils/res_utils.py `resize`)"""
    lib = load()
    x = _f32c(x.detach())
    M, N = x.shape[-2], x.shape[-1]
    Mo, No = int(out_size[0]), int(out_size[1])
    rows = x.numel() // (M * N)
    out = torch.empty(*x.shape[:-2], Mo, No, dtype=torch.float32, device=x.device)
    run("resize2d", lib.rpde_resize2d_ws_bytes(rows, M, N, Mo, No), x.device, ptr(x), ptr(out), rows, M, N, Mo, No)
    return out


# ----------------------------------------------------------------------------
# error by frequency (evaluators: no autograd).  Reference utils/frequency_error.py decompose_error_by_frequency_1d /
# _2d take one inverse FFT and one .item() per mode or bin; here it is one call that ADDS the batch's error and solution
# energy per mode / radial bin into a float64 device accumulator (csrc/freq_energy.hip) -- sqrt of it is the reference's
# magnitude -- so a test set streams through in batches with no host synchronisation.
# ----------------------------------------------------------------------------
_RADIAL_BINS: dict = {}


def radial_bins(H: int, W: int, num_radial_bins: int = 64):
    """(bins, centres): bins int32 [H, W//2+1], the radial frequency bin of every rfft2 entry or -1 (entries with
    r >= 0.5, the corners and the on-axis Nyquist lines, belong to no bin); centres float64 [num_radial_bins].  Built
    with the reference's dtypes -- r a float32 tensor, edges np.linspace in float64, membership edges[i] <= r <
    edges[i+1] -- so that entries on an edge fall where the reference puts them.  Host tensors, cached."""
    import numpy as np
    key = (int(H), int(W), int(num_radial_bins))
    hit = _RADIAL_BINS.get(key)
    if hit is not None:
        return hit
    if key[2] < 1 or key[0] < 2 or key[1] < 2:
        raise ValueError(f"radial_bins: bad H={H} W={W} num_radial_bins={num_radial_bins}")
    fy = torch.fft.fftfreq(key[0]).view(-1, 1)
    fx = torch.fft.rfftfreq(key[1]).view(1, -1)
    r = torch.sqrt(fy ** 2 + fx ** 2)
    edges = np.linspace(0, 0.5, key[2] + 1)
    bins = torch.full(r.shape, -1, dtype=torch.int32)
    for i in range(key[2]):
        bins[(r >= edges[i]) & (r < edges[i + 1])] = i
    assert int(bins.min()) >= -1 and int(bins.max()) < key[2]       # the kernel trusts this range
    centres = (edges[:-1] + edges[1:]) / 2
    _RADIAL_BINS[key] = (bins.contiguous(), centres)
    return _RADIAL_BINS[key]


_RADIAL_BINS_DEV: dict = {}


def _radial_bins_on(device, H: int, W: int, nb: int) -> torch.Tensor:
    key = (torch.device(device), int(H), int(W), int(nb))
    t = _RADIAL_BINS_DEV.get(key)
    if t is None:
        t = _RADIAL_BINS_DEV[key] = radial_bins(H, W, nb)[0].to(device)
    return t


def _channels_first(t: torch.Tensor, channels_last: bool) -> torch.Tensor:
    """[B, ..., C] -> [B, C, ...]: a view when C == 1, otherwise a permuted copy made by _f32c"""
    if not channels_last:
        return t
    if t.shape[-1] == 1:
        return t.reshape(t.shape[0], 1, *t.shape[1:-1]) if t.is_contiguous() else t.movedim(-1, 1)
    return t.movedim(-1, 1)


def _freq_acc(acc, n_out: int, device) -> torch.Tensor:
    if acc is None:
        return torch.zeros(2, n_out, dtype=torch.float64, device=device)
    if acc.dtype != torch.float64 or tuple(acc.shape) != (2, n_out) or not acc.is_contiguous() or acc.device != device:
        raise ValueError(f"acc must be a contiguous float64 [2, {n_out}] tensor on {device}")
    return acc


def freq_energy1d(pred: torch.Tensor, target: torch.Tensor, acc: Optional[torch.Tensor] = None,
                  num_modes: Optional[int] = None, channels_last: bool = False) -> torch.Tensor:
    """pred, target [B, C, n] (channels_last: [B, n, C]).  Adds into acc [2, num_modes] float64 (created zeroed when
    None) and returns it: acc[0, k] += w_k / n sum_{b,c} |rfft(pred - target)[b,c,k]|^2, acc[1, k] the same of target;
    the difference is formed in fp32 before the transform.  num_modes (None or 0: all) is clamped to n // 2 + 1."""
    lib = load()
    if pred.shape != target.shape or pred.dim() != 3:
        raise ValueError(f"freq_energy1d: pred {tuple(pred.shape)} / target {tuple(target.shape)}, expected equal 3-D shapes")
    p = _f32c(_channels_first(pred.detach(), channels_last))
    t = _f32c(_channels_first(target.detach(), channels_last))
    n = p.shape[-1]
    rows = p.numel() // n
    k = min(int(num_modes or n // 2 + 1), n // 2 + 1)             # None or 0: every mode, as the reference's `or`
    acc = _freq_acc(acc, k, p.device)
    run("freq_energy1d", lib.rpde_freq_energy1d_ws_bytes(rows, n, k), p.device, ptr(p), ptr(t), acc.data_ptr(), rows,
        n, k)
    return acc


def freq_energy2d(pred: torch.Tensor, target: torch.Tensor, num_radial_bins: int = 64,
                  acc: Optional[torch.Tensor] = None, channels_last: bool = False) -> torch.Tensor:
    """pred, target [B, C, H, W] (channels_last: [B, H, W, C]).  Adds into acc [2, num_radial_bins] float64 and returns
    it: acc[0, i] += 1/(H W) sum_{(ky,kx) in bin i} w_kx sum_{b,c} |rfft2(pred - target)[b,c,ky,kx]|^2, acc[1, i] the
    same of target; bins as radial_bins() defines them."""
    lib = load()
    if pred.shape != target.shape or pred.dim() != 4:
        raise ValueError(f"freq_energy2d: pred {tuple(pred.shape)} / target {tuple(target.shape)}, expected equal 4-D shapes")
    p = _f32c(_channels_first(pred.detach(), channels_last))
    t = _f32c(_channels_first(target.detach(), channels_last))
    H, W = p.shape[-2], p.shape[-1]
    images = p.numel() // (H * W)
    nb = int(num_radial_bins)
    bins = _radial_bins_on(p.device, H, W, nb)
    acc = _freq_acc(acc, nb, p.device)
    run("freq_energy2d", lib.rpde_freq_energy2d_ws_bytes(images, H, W), p.device, ptr(p), ptr(t), bins.data_ptr(),
        acc.data_ptr(), images, H, W, nb)
    return acc


# ----------------------------------------------------------------------------
# per-sample, per-band spectral energies with autograd (csrc/band_energy.hip, rpde_band_energy_*): the primitive under
# utils.loss.BandRelativeL2Loss / SpectrumMatchingLoss and utils.autoregressive_step.rollout_band_energy.  GPU tensors
# only, no CPU fallback.
# ----------------------------------------------------------------------------
_BAND_TABLES: dict = {}
_BAND_TABLES_DEV: dict = {}
BAND_KINDS = ("octave", "radial", "modes")
MAX_BANDS = 4096


def _band_grid(spatial_shape, what: str):
    """(grid, M, N) of a 1-D (n,) or 2-D (H, W) grid; M = 1 in 1-D"""
    grid = tuple(int(n) for n in spatial_shape)
    if len(grid) not in (1, 2) or min(grid) < 2:
        raise ValueError(f"{what}: spatial_shape {tuple(spatial_shape)}, expected (n,) or (H, W) with every axis >= 2")
    return grid, (1 if len(grid) == 1 else grid[0]), grid[-1]


def band_table(spatial_shape, kind: str, num_bands: Optional[int] = None):
    """(table, J): table int32 [M, N//2+1] (M = 1 for a 1-D grid), the band in -1 .. J-1 of every rfft / rfft2 entry,
    rows in fft order.  Host tensors, cached.
      "octave"  band 0 for k = 0, else 1 + floor(log2 |k|), |k|^2 = k1^2 + k2^2 with signed integer wavenumbers (k1 = 0
                in 1-D), in integer arithmetic (1 + (bit_length(|k|^2) - 1) // 2: exact on the band edges).  Every entry
                has a band and a band means the same physical scales at every resolution; J follows from the grid.
      "radial"  (2-D) radial_bins(H, W, num_bands)[0] unchanged, num_bands = 64 by default: the evaluator's bins, entries
                with r >= 0.5 stay -1.
      "modes"   (1-D) band = mode index for k < num_bands, -1 above."""
    grid, M, N = _band_grid(spatial_shape, "band_table")
    key = (grid, str(kind), None if num_bands is None else int(num_bands))
    hit = _BAND_TABLES.get(key)
    if hit is not None:
        return hit
    K = N // 2 + 1
    if kind == "octave":
        if num_bands is not None:
            raise ValueError("band_table: the octave bands follow from the grid, num_bands must be None")
        k1 = torch.arange(M, dtype=torch.int64)
        k1 = torch.where(k1 <= (M - 1) // 2, k1, k1 - M)
        k2 = torch.arange(K, dtype=torch.int64)
        q = k1.view(-1, 1) ** 2 + k2.view(1, -1) ** 2
        bits, v = torch.zeros_like(q), q.clone()
        while bool(v.any()):                                   # bit_length, entry by entry
            bits += (v > 0).to(torch.int64)
            v >>= 1
        table = torch.where(q == 0, torch.zeros_like(q), 1 + (bits - 1) // 2)
        J = int(table.max()) + 1
    elif kind == "radial":
        if len(grid) != 2:
            raise ValueError("band_table: radial bands are for 2-D grids")
        J = 64 if num_bands is None else int(num_bands)
        table = radial_bins(M, N, J)[0]
    elif kind == "modes":
        if len(grid) != 1 or num_bands is None or int(num_bands) < 1:
            raise ValueError("band_table: 'modes' is for 1-D grids and needs num_bands >= 1")
        J = int(num_bands)
        k2 = torch.arange(K, dtype=torch.int64).view(1, K)
        table = torch.where(k2 < J, k2, torch.full_like(k2, -1))
    else:
        raise ValueError(f"band_table: unknown kind {kind!r} (kinds: {', '.join(BAND_KINDS)})")
    if not 1 <= J <= MAX_BANDS:
        raise ValueError(f"band_table: {J} bands, expected 1 .. {MAX_BANDS}")
    _BAND_TABLES[key] = (table.to(torch.int32).reshape(M, K).contiguous(), J)
    return _BAND_TABLES[key]


def check_band_table(table: torch.Tensor, spatial_shape, J: int) -> None:
    """ValueError unless table is an integer table of the half spectrum of this grid ([M, N//2+1]; [N//2+1] also for a
    1-D grid) with values in -1 .. J-1 whose self-conjugate columns (kx = 0 and, for even W, kx = W/2) are symmetric
    in ky: otherwise gE[band] * rfft2(z) is not the spectrum of a real field and the inverse transform is not the
    gradient"""
    grid, M, N = _band_grid(spatial_shape, "check_band_table")
    K = N // 2 + 1
    if not torch.is_tensor(table) or table.is_floating_point() or table.is_complex() or table.dtype == torch.bool:
        raise ValueError(f"band table: expected an integer tensor, got {getattr(table, 'dtype', type(table))}")
    ok = ((M, K),) + (((K,),) if M == 1 else ())
    if tuple(table.shape) not in ok:
        raise ValueError(f"band table of shape {tuple(table.shape)}: the grid {grid} needs {(M, K)}")
    if not 1 <= int(J) <= MAX_BANDS:
        raise ValueError(f"band table: {J} bands, expected 1 .. {MAX_BANDS}")
    t = table.detach().cpu().to(torch.int64).reshape(M, K)
    if int(t.min()) < -1 or int(t.max()) >= int(J):
        raise ValueError(f"band table: values {int(t.min())} .. {int(t.max())}, expected -1 .. {int(J) - 1}")
    if M > 1:
        flip = (M - torch.arange(M)) % M
        for kx in [0] + ([N // 2] if N % 2 == 0 else []):
            if not torch.equal(t[:, kx], t[flip, kx]):
                raise ValueError(f"band table: column kx={kx} is not symmetric in ky (band[ky] != band[(H - ky) % H])")


class BandTables:
    """the device tables of one (grid, band table): what rpde_band_energy_* take (include/rpde.h)"""
    __slots__ = ("grid", "J", "J_e", "n_entries", "band", "entries", "start")

    def __init__(self, grid, J, J_e, n_entries, band, entries, start):
        self.grid, self.J, self.J_e, self.n_entries = grid, J, J_e, n_entries
        self.band, self.entries, self.start = band, entries, start


def band_tables(table: torch.Tensor, J: int, spatial_shape, device) -> BandTables:
    """Validate a host band table and build its device forms: the padded band-of-every-entry table [M, kp] and the
    entries of each band listed band by band (ky-major inside a band) with start [J+1].  J_e: bands that own at least
    one entry.  One host pass and three copies: callers keep the result per (grid, device)."""
    check_band_table(table, spatial_shape, J)
    grid, M, N = _band_grid(spatial_shape, "band_tables")
    J, K, kp = int(J), N // 2 + 1, _kp(N)
    t = table.detach().cpu().to(torch.int64).reshape(M, K)
    band = torch.full((M, kp), -1, dtype=torch.int32)
    band[:, :K] = t.to(torch.int32)
    ky = torch.arange(M, dtype=torch.int64).view(M, 1)
    kx = torch.arange(K, dtype=torch.int64).view(1, K)
    twice = ~((kx == 0) | ((kx == N // 2) & (N % 2 == 0)))
    packed = (((ky * (2 * kp) + kx) << 1) | twice.to(torch.int64)).reshape(-1)
    flat = t.reshape(-1)
    keep = flat >= 0
    order = torch.argsort(flat[keep], stable=True)
    entries = packed[keep][order].to(torch.int32)
    counts = torch.bincount(flat[keep], minlength=J)
    start = torch.zeros(J + 1, dtype=torch.int32)
    start[1:] = torch.cumsum(counts, 0).to(torch.int32)
    n = int(entries.numel())
    if n == 0:
        entries = torch.zeros(1, dtype=torch.int32)              # a pointer to pass; no entry is read
    return BandTables(grid, J, int((counts > 0).sum()), n, band.to(device), entries.to(device), start.to(device))


def _band_tables_on(device, grid, kind: str, num_bands) -> BandTables:
    key = (torch.device(device), tuple(grid), str(kind), None if num_bands is None else int(num_bands))
    t = _BAND_TABLES_DEV.get(key)
    if t is None:
        table, J = band_table(grid, kind, num_bands)
        t = _BAND_TABLES_DEV[key] = band_tables(table, J, grid, device)
    return t


def resolve_bands(bands, spatial_shape, device) -> BandTables:
    """the device tables of what band_energy accepts as `bands`, for this grid: a kind and (kind, num_bands) come from
    the cache, an integer table is validated and copied, BandTables pass through"""
    grid = tuple(int(n) for n in spatial_shape)
    if isinstance(bands, BandTables):
        T = bands
    elif isinstance(bands, str):
        T = _band_tables_on(device, grid, bands, None)
    elif isinstance(bands, (tuple, list)) and len(bands) == 2 and isinstance(bands[0], str):
        T = _band_tables_on(device, grid, bands[0], bands[1])
    elif torch.is_tensor(bands):
        T = band_tables(bands, max(int(bands.max()), 0) + 1 if bands.numel() else 1, grid, device)
    else:
        raise ValueError("bands must be a kind, (kind, num_bands), an integer table or BandTables")
    if T.grid != grid:
        raise ValueError(f"band tables of the grid {T.grid} for a field on {grid}")
    return T


class _BandEnergy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, T: BandTables, dims: int):
        lib = load()
        x = _f32c(x)
        px = ptr(x)                                            # raises for CPU tensors: there is no fallback
        py = None
        if y is not None:
            if y.shape != x.shape:
                raise ValueError(f"band_energy: x {tuple(x.shape)} / y {tuple(y.shape)} differ")
            y = _f32c(y)
            py = ptr(y)
        B, Cc, M, N = _bcmn(x, dims)
        if T.band.device != x.device:
            raise ValueError(f"band_energy: band tables on {T.band.device}, x on {x.device}")
        nws = lib.rpde_band_energy_ws_bytes(B, Cc, M, N, T.J)
        if nws == 0:
            raise ValueError(f"band_energy: unsupported B={B} C={Cc} grid {tuple(x.shape[2:])} J={T.J}")
        keep = ctx.needs_input_grad[0]
        E = torch.empty(B, T.J, dtype=torch.float32, device=x.device)
        spec = torch.empty(lib.rpde_band_energy_spec_elems(B, Cc, M, N), dtype=torch.float32, device=x.device) if keep else None
        run("band_energy_fwd", nws, x.device, px, py, T.entries.data_ptr(), T.start.data_ptr(), T.n_entries, ptr(E),
            ptr(spec), B, Cc, M, N, T.J)
        if keep:
            ctx.save_for_backward(spec)
        ctx.meta = (tuple(x.shape), B, Cc, M, N, T)
        return E

    @staticmethod
    def backward(ctx, gE):
        lib = load()
        spec, = ctx.saved_tensors
        shape, B, Cc, M, N, T = ctx.meta
        gE = _f32c(gE)
        gx = torch.empty(shape, dtype=torch.float32, device=spec.device)
        run("band_energy_bwd", lib.rpde_band_energy_ws_bytes(B, Cc, M, N, T.J), spec.device, ptr(spec),
            T.band.data_ptr(), ptr(gE), ptr(gx), B, Cc, M, N, T.J)
        return gx, None, None, None


def band_energy(x, bands, dims: int, y=None):
    """E [B, J] fp32: E[b, j] = sum_c sum_{(ky,kx) in band j} c_kx / (M N) |rfft(z)[b,c,ky,kx]|^2 (rfft2 for dims=2) of
    z = x, or z = x - y formed in fp32 before the transform; c_kx the Hermitian multiplicity of the half axis.  x, y:
    channels-first [B, C, n] / [B, C, H, W] fp32 tensors on the GPU.  bands: a kind of band_table ("octave"), a pair
    (kind, num_bands), an integer table for this grid (its J is max + 1; validated and copied on every call), or the
    BandTables that band_tables() prepared.  Gradient for x only; the spectrum is kept only when x needs one."""
    if dims not in (1, 2):
        raise ValueError(f"band_energy: dims must be 1 or 2, got {dims}")
    if x.dim() != dims + 2:
        raise ValueError(f"band_energy: x {tuple(x.shape)}, expected a {dims + 2}-D channels-first tensor")
    if not x.is_cuda:
        ptr(x)                                                 # the CPU refusal of every op
    return _BandEnergy.apply(x, y, resolve_bands(bands, x.shape[2:], x.device), int(dims))


# ----------------------------------------------------------------------------
# Navier-Stokes vorticity generator and its Gaussian random field (csrc/ns_solver.hip, rpde_ns2d_* / rpde_grf2d;
# data_generation/ns_2d.py and random_fields.py are the callers).  Data production: no autograd, GPU tensors only,
# no CPU fallback.
# ----------------------------------------------------------------------------
def _kp(N: int) -> int:
    """padded length of a half spectrum's contiguous axis: N//2+1 rounded up to 4 (csrc/halfspec.h)"""
    return (N // 2 + 1 + 3) // 4 * 4


def _grid(t: torch.Tensor, what: str, d: int):
    """the dims of a batch of d-dimensional fields, [B, N] or [B, M, N], refused as the C side refuses them"""
    names = ("B", "N") if d == 1 else ("B", "M", "N")
    if t.dim() != d + 1:
        raise ValueError(f"{what}: expected [{', '.join(names)}], got {tuple(t.shape)}")
    dims = tuple(int(v) for v in t.shape)
    if (load().rpde_etd1d_ws_bytes if d == 1 else load().rpde_ns2d_ws_bytes)(*dims) == 0:
        raise ValueError(f"{what}: unsupported grid {' '.join(f'{n}={v}' for n, v in zip(names, dims))} "
                         + ("(N even, 4 .. 4096, B <= 65535)" if d == 1 else "(even axes 4 .. 4096)"))
    return dims


def _padded(t: torch.Tensor) -> torch.Tensor:
    """a float64 table [..., K] of a half spectrum's K = N//2+1 columns -> float32 [..., kp], rounded once, padding zero"""
    K = t.shape[-1]
    p = torch.zeros(*t.shape[:-1], _kp(2 * (K - 1)), dtype=torch.float32)
    p[..., :K] = t.to(torch.float32)
    return p


def _schedule(what: str, steps, record_every):
    """(steps, record_every) as ints, refused unless steps >= 0 and record_every >= 1"""
    steps, record_every = int(steps), int(record_every)
    if steps < 0 or record_every < 1:
        raise ValueError(f"{what}: bad steps={steps} record_every={record_every}")
    return steps, record_every


def _grf(what: str, d: int, noise: torch.Tensor, sqrt_eig: torch.Tensor) -> torch.Tensor:
    """noise [B, *grid, 2], sqrt_eig [*grid] of d dimensions -> [B, *grid] through rpde_grf1d / rpde_grf2d"""
    lib = load()
    if noise.dim() != d + 2 or noise.shape[-1] != 2 or tuple(sqrt_eig.shape) != tuple(noise.shape[1:-1]):
        raise ValueError(f"{what}: noise {tuple(noise.shape)} / sqrt_eig {tuple(sqrt_eig.shape)}, expected "
                         + ("[B, N, 2] and [N]" if d == 1 else "[B, M, N, 2] and [M, N]"))
    noise, sqrt_eig = _f32c(noise.detach()), _f32c(sqrt_eig.detach())
    pn, ps = ptr(noise), ptr(sqrt_eig)                     # raises for CPU tensors: there is no fallback
    dims = _grid(noise[..., 0], what, d)
    out = torch.empty(dims, dtype=torch.float32, device=noise.device)
    run(what, getattr(lib, f"rpde_{what}_ws_bytes")(*dims), noise.device, pn, ps, ptr(out), *dims)
    return out


def _ns2d_symbols(M: int, N: int):
    """(lap, dealias, poisson): float64 [M, K] tables of the half spectrum of an M x N grid, K = N//2+1 -- k1 = fftfreq(M) M
    (signed, Nyquist -M/2), k2 = 0 .. N/2, lap = 4 pi^2 (k1^2 + k2^2), dealias = |k1| <= (2/3)(M/2) and |k2| <= (2/3)(N/2),
    poisson = lap with the mean mode's entry set to 1"""
    import math
    M, N = int(M), int(N)
    K = N // 2 + 1
    k1 = (torch.fft.fftfreq(M, dtype=torch.float64) * M).round().view(M, 1)
    k2 = torch.arange(K, dtype=torch.float64).view(1, K)
    lap = 4.0 * math.pi ** 2 * (k1 ** 2 + k2 ** 2)
    dealias = ((k1.abs() <= (2.0 / 3.0) * (M // 2)) & (k2.abs() <= (2.0 / 3.0) * (N // 2))).to(torch.float64)
    poisson = lap.clone()
    poisson[0, 0] = 1.0
    return lap, dealias, poisson


def ns2d_tables(M: int, N: int, visc: float, dt: float):
    """(c_w, c_f, c_g, inv_lap): the step's coefficient tables, float32 [M, kp] host tensors (kp = N//2+1 rounded up to
    4, padded columns zero), formed in float64 and rounded once.  k1 = fftfreq(M) M (signed, Nyquist -M/2),
    k2 = 0 .. N/2, lap = 4 pi^2 (k1^2 + k2^2), a = dt visc lap / 2, dealias = |k1| <= (2/3)(M/2) and |k2| <= (2/3)(N/2):
    c_w = (1 - a)/(1 + a), c_f = dt dealias/(1 + a), c_g = dt/(1 + a), inv_lap = 1/lap with the mean mode's lap set to
    1 for this division only."""
    lap, dealias, poisson = _ns2d_symbols(M, N)
    a = 0.5 * float(dt) * float(visc) * lap
    return tuple(_padded(t) for t in ((1.0 - a) / (1.0 + a), float(dt) * dealias / (1.0 + a), float(dt) / (1.0 + a),
                                      1.0 / poisson))


def grf2d(noise: torch.Tensor, sqrt_eig: torch.Tensor) -> torch.Tensor:
    """noise [B, M, N, 2] (real and imaginary part of the coefficients of the full M x N grid, standard normal),
    sqrt_eig [M, N] -> [B, M, N] = Re ifft2(sqrt_eig . noise), torch's 1/(M N) included.  The HIP side is deterministic
    given the noise.  Contiguous fp32 tensors on the GPU; no autograd, no CPU fallback."""
    return _grf("grf2d", 2, noise, sqrt_eig)


def _ns2d_forcing(what: str, f: torch.Tensor, c_g: torch.Tensor, B: int, M: int, N: int, ws: torch.Tensor, nws: int):
    """(g_h, batched): g_h = dt / (1 + a) rfft2(f) for the forcing f [M, N] (one for the batch) or [B, M, N], once per
    solve, and whether it holds a spectrum per sample"""
    lib = load()
    if tuple(f.shape) not in ((M, N), (B, M, N)):
        raise ValueError(f"{what}: forcing {tuple(f.shape)}, expected {(M, N)} or {(B, M, N)}")
    fb = 1 if f.dim() == 2 else B
    st = stream_ptr()
    # The forcing is transformed one image at a time, so that a sample's forcing spectrum does not depend on the batch
    # around it: f [M, N] and the same f repeated B times give the same bits
    per = lib.rpde_ns2d_spec_elems(1, M, N)
    f_h = torch.empty(fb * per, dtype=torch.float32, device=c_g.device)
    g_h = torch.empty_like(f_h)
    f3 = f.view(fb, M, N)
    for i in range(fb):
        run("ns2d_rfft2", nws, ws, ptr(f3[i]), ptr(f_h[i * per:(i + 1) * per]), 1, M, N)
    check(lib.rpde_ns2d_scale(ptr(f_h), ptr(c_g), ptr(g_h), fb, M, N, st), "ns2d_scale")
    return g_h, int(f.dim() == 3)


def ns2d_solve(w0: torch.Tensor, f: torch.Tensor, visc: float, dt: float, steps: int, record_every: int) -> torch.Tensor:
    """2-D Navier-Stokes in vorticity form on the periodic unit square from w0 [B, M, N] with forcing f ([M, N] for the
    whole batch or [B, M, N]): `steps` pseudo-spectral steps of size dt (Crank-Nicolson diffusion, explicit advection and
    forcing, 2/3 de-aliasing; include/rpde.h has the formulas), a snapshot after every `record_every`-th.  Returns
    [B, M, N, steps // record_every].  Six launches per step, no host synchronisation between them.  Contiguous fp32
    tensors on the GPU; no autograd, no CPU fallback."""
    lib = load()
    steps, record_every = _schedule("ns2d_solve", steps, record_every)
    w0, f = _f32c(w0.detach()), _f32c(f.detach())
    pw, _ = ptr(w0), ptr(f)                                # raises for CPU tensors: there is no fallback
    B, M, N = _grid(w0, "ns2d_solve", 2)
    dev = w0.device
    c_w, c_f, c_g, inv_lap = (t.to(dev) for t in ns2d_tables(M, N, visc, dt))
    nws = lib.rpde_ns2d_ws_bytes(B, M, N)
    ws = workspace(nws, dev)                               # one workspace for every call of the solve
    g_h, batched = _ns2d_forcing("ns2d_solve", f, c_g, B, M, N, ws, nws)
    W = torch.empty(lib.rpde_ns2d_spec_elems(B, M, N), dtype=torch.float32, device=dev)
    run("ns2d_rfft2", nws, ws, pw, ptr(W), B, M, N)
    n_rec = steps // record_every
    snaps = torch.empty(max(n_rec, 1), B, M, N, dtype=torch.float32, device=dev)
    for c in range(n_rec):
        run("ns2d_steps", nws, ws, ptr(W), ptr(g_h), batched, ptr(c_w), ptr(c_f), ptr(inv_lap), B, M, N, record_every)
        run("ns2d_irfft2", nws, ws, ptr(W), ptr(snaps[c]), B, M, N)
    return snaps[:n_rec].permute(1, 2, 3, 0).contiguous()


# ----------------------------------------------------------------------------
# Active-scalar Navier-Stokes generator (csrc/ns_solver.hip, rpde_nsc2d_*; data_generation/active_scalar_2d.py is the
# caller).  Data production: no autograd, GPU tensors only, no CPU fallback.
# ----------------------------------------------------------------------------
def nsc2d_tables(M: int, N: int, visc: float, kappa: float, dt: float):
    """(c_w, c_f, d_w, d_f, c_g, inv_lap): the coupled step's coefficient tables, float32 [M, kp] host tensors with the
    padded columns zero -- ns2d_tables' arithmetic, once with the viscosity (c_w, c_f, c_g, inv_lap) and once with the
    scalar's diffusivity, b = dt kappa lap / 2: d_w = (1 - b)/(1 + b), d_f = dt dealias/(1 + b)."""
    c_w, c_f, c_g, inv_lap = ns2d_tables(M, N, visc, dt)
    d_w, d_f, _, _ = ns2d_tables(M, N, kappa, dt)
    return c_w, c_f, d_w, d_f, c_g, inv_lap


def _nsc2d_state(what: str, w: torch.Tensor, c: torch.Tensor):
    """w, c [B, M, N] -> (lib, B, M, N, ws, nws, S): S = [rfft2(w), rfft2(c)], the solver's state of 2 B half spectra"""
    lib = load()
    w, c = _f32c(w.detach()), _f32c(c.detach())
    ptr(w), ptr(c)                                         # raises for CPU tensors: there is no fallback
    B, M, N = _grid(w, what, 2)
    if tuple(c.shape) != (B, M, N) or c.device != w.device:
        raise ValueError(f"{what}: scalar {tuple(c.shape)} on {c.device}, expected {(B, M, N)} on {w.device}")
    nws = lib.rpde_nsc2d_ws_bytes(B, M, N)
    if nws == 0:
        raise ValueError(f"{what}: unsupported batch B={B} for the grid {M} x {N} (6 B <= 65535, 24 B max(M, N) < 2^31)")
    ws = workspace(nws, w.device)
    S = torch.empty(lib.rpde_ns2d_spec_elems(2 * B, M, N), dtype=torch.float32, device=w.device)
    wc = torch.cat([w, c], dim=0)
    run("ns2d_rfft2", nws, ws, ptr(wc), ptr(S), 2 * B, M, N)
    return lib, B, M, N, ws, nws, S


def nsc2d_fields(w: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    """w (vorticity), c (scalar) [B, M, N] -> [B, 3, M, N] = (c, q, v): the scalar and the velocity u = (q, v) of w,
    q = d psi/dx2, v = -d psi/dx1, lap psi = -w, through rpde_nsc2d_fields (c itself goes through the transform pair).
    Contiguous fp32 tensors on the GPU; no autograd, no CPU fallback."""
    lib, B, M, N, ws, nws, S = _nsc2d_state("nsc2d_fields", w, c)
    inv_lap = ns2d_tables(M, N, 0.0, 0.0)[3].to(S.device)
    out = torch.empty(B, 3, M, N, dtype=torch.float32, device=S.device)
    run("nsc2d_fields", nws, ws, ptr(S), ptr(inv_lap), ptr(out), B, M, N)
    return out


def nsc2d_solve(w0: torch.Tensor, c0: torch.Tensor, f: torch.Tensor, visc: float, kappa: float, beta: float, dt: float,
                steps: int, record_every: int):
    """2-D Navier-Stokes in vorticity form with an active scalar on the periodic unit square: from w0, c0 [B, M, N] with
    forcing f ([M, N] or [B, M, N]) on the vorticity, `steps` pseudo-spectral steps of size dt of
        w_t + u . grad w = visc lap w + beta dc/dx1 + f,    c_t + u . grad c = kappa lap c
    (Crank-Nicolson on both diffusions, explicit advection, buoyancy and forcing, 2/3 de-aliasing; include/rpde.h has the
    formulas), a snapshot after every `record_every`-th.  Returns (fields [B, steps // record_every, 3, M, N] = (c, q, v)
    with u = (q, v), vorticity [B, steps // record_every, M, N]).  Six launches per step, one device call per snapshot's
    steps, no host synchronisation.  Contiguous fp32 tensors on the GPU; no autograd, no CPU fallback."""
    steps, record_every = _schedule("nsc2d_solve", steps, record_every)
    f = _f32c(f.detach())
    ptr(f)
    lib, B, M, N, ws, nws, S = _nsc2d_state("nsc2d_solve", w0, c0)
    dev = S.device
    c_w, c_f, d_w, d_f, c_g, inv_lap = (t.to(dev) for t in nsc2d_tables(M, N, visc, kappa, dt))
    g_h, batched = _ns2d_forcing("nsc2d_solve", f, c_g, B, M, N, ws, nws)
    n_rec = steps // record_every
    fields = torch.empty(max(n_rec, 1), B, 3, M, N, dtype=torch.float32, device=dev)
    vort = torch.empty(max(n_rec, 1), B, M, N, dtype=torch.float32, device=dev)
    for c in range(n_rec):
        run("nsc2d_steps", nws, ws, ptr(S), ptr(g_h), batched, ptr(c_w), ptr(c_f), ptr(d_w), ptr(d_f), ptr(inv_lap),
            float(beta), B, M, N, record_every)
        run("nsc2d_fields", nws, ws, ptr(S), ptr(inv_lap), ptr(fields[c]), B, M, N)
        run("ns2d_irfft2", nws, ws, ptr(S), ptr(vort[c]), B, M, N)
    return fields[:n_rec].transpose(0, 1).contiguous(), vort[:n_rec].transpose(0, 1).contiguous()


# ----------------------------------------------------------------------------
# 1-D exponential-time-differencing generator and the 1-D Gaussian random field (csrc/etd1d.hip, rpde_etd1d_* /
# rpde_grf1d; data_generation/burgers_1d.py, ks_1d.py and random_fields.py are the callers).  Data production: no
# autograd, GPU tensors only, no CPU fallback.
# ----------------------------------------------------------------------------
def _contour(z: torch.Tensor, full_circle: bool):
    """(LR, mean): LR = z[..., None] + r_m over the Kassam-Trefethen contour points r_m -- the 32 points of the upper half
    circle with Re<.> of the mean for real z, the full circle's 64 points with the complex mean otherwise -- and the
    mean over them, for z of any shape"""
    import math
    points = 64 if full_circle else 32
    m = torch.arange(1, points + 1, dtype=torch.float64)
    r = torch.polar(torch.ones(points, dtype=torch.float64), (2.0 if full_circle else 1.0) * math.pi * (m - 0.5) / points)
    LR = z.unsqueeze(-1).to(torch.complex128) + r

    def mean(t):
        return t.mean(dim=-1) if full_circle else t.mean(dim=-1).real

    return LR, mean


def _etd1d_contour(what: str, N, length, dt, symbol, advect, dealias, full_circle: bool):
    """What every table of the 1-D ETD family starts from: z = dt symbol(kappa) [K], LR = z + r_m [K, points] over the
    Kassam-Trefethen contour points r_m, the mean over them and the float64 g [K].  For real z the 32 points of the upper
    half circle, exp(i pi (m - 1/2) / 32), with Re<.> of the mean; for complex z that is wrong, and it is the full
    circle's 64 points, exp(2 pi i (m - 1/2) / 64), with the complex mean."""
    import math
    N = int(N)
    if N < 4 or N % 2:
        raise ValueError(f"{what}: N must be even and >= 4, got {N}")
    if not (float(length) > 0 and float(dt) > 0):
        raise ValueError(f"{what}: length and dt must be positive, got length={length} dt={dt}")
    K = N // 2 + 1
    n = torch.arange(K, dtype=torch.float64)
    kappa = (2.0 * math.pi / float(length)) * n
    z = float(dt) * symbol(kappa)
    LR, mean = _contour(z, full_circle)
    keep = (n <= (2.0 / 3.0) * (N // 2)).to(torch.float64) if dealias else torch.ones(K, dtype=torch.float64)
    g = -(float(advect) / 2.0) * kappa * keep
    g[N // 2] = 0.0
    return z, LR, mean, g


def _etd1d_tables(what: str, N, length, dt, symbol, advect, dealias, full_circle: bool):
    """The tables under etd1d_tables (full_circle False) and etd1d_tables_cx (True): six float64 / complex128
    coefficients [K] of z = dt symbol(kappa) and the float32 [kp] table g, on the contour of _etd1d_contour."""
    z, LR, mean, g = _etd1d_contour(what, N, length, dt, symbol, advect, dealias, full_circle)
    h = float(dt)
    eLR = torch.exp(LR)
    coefficients = (torch.exp(z), torch.exp(z / 2.0),
                    h * mean((torch.exp(LR / 2.0) - 1.0) / LR),
                    h * mean((-4.0 - LR + eLR * (4.0 - 3.0 * LR + LR ** 2)) / LR ** 3),
                    h * mean((2.0 + LR + eLR * (-2.0 + LR)) / LR ** 3),
                    h * mean((-4.0 - 3.0 * LR - LR ** 2 + eLR * (4.0 - LR)) / LR ** 3))
    return z, coefficients, _padded(g)


def _cx_symbol(c1, c2, c3, c4):
    """kappa [K] -> l = c2 kappa^2 + c4 kappa^4 + i (c1 kappa + c3 kappa^3) with Im l_{N/2} = 0"""
    def symbol(kappa):
        odd = float(c1) * kappa + float(c3) * kappa ** 3
        odd[-1] = 0.0
        return torch.complex(float(c2) * kappa ** 2 + float(c4) * kappa ** 4, odd)
    return symbol


def _cx_padded(z: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    """a complex128 table [K] of z -> float32 [2, kp] (real plane, imaginary plane).  Real z (the mean and Nyquist modes,
    an even symbol): the circle's points pair up as conjugates and the mean is real; what its imaginary part holds then
    is the sum's rounding (1e-20), dropped"""
    return _padded(torch.stack([t.real, torch.where(z.imag == 0, torch.zeros_like(t.imag), t.imag)]))


def etd1d_tables(N: int, length: float, c2: float, c4: float, dt: float, advect: float = 1.0, dealias: bool = True):
    """(E, E2, Q, f1, f2, f3, g): the ETDRK4 tables of u_t = L u - (advect/2) (u^2)_x with the symbol
    l_n = c2 kappa_n^2 + c4 kappa_n^4, kappa_n = 2 pi n / length, as float32 [kp] host tensors (kp = N//2+1 rounded up to
    4, padding zero), formed in float64 and rounded once.  Kassam-Trefethen: z = dt l_n, LR = z + r_m on the 32 contour
    points r_m = exp(i pi (m - 1/2) / 32) -- the f coefficients cancel catastrophically in fp32 for small z, the contour
    mean in float64 does not.  g_n = -(advect/2) kappa_n dealias_n, dealias_n = [n <= (2/3)(N/2)] (or 1), g_{N/2} = 0.
    include/rpde.h has the formulas."""
    _, coefficients, g = _etd1d_tables("etd1d_tables", N, length, dt,
                                       lambda kappa: float(c2) * kappa ** 2 + float(c4) * kappa ** 4, advect, dealias, False)
    return tuple(_padded(t) for t in coefficients) + (g,)


def etd1d_tables_cx(N: int, length: float, c1: float, c2: float, c3: float, c4: float, dt: float, advect: float = 1.0,
                    dealias: bool = True):
    """(E, E2, Q, f1, f2, f3, g): the ETDRK4 tables of u_t = L u - (advect/2) (u^2)_x for a symbol with odd derivatives,
    l_n = c2 kappa_n^2 + c4 kappa_n^4 + i (c1 kappa_n + c3 kappa_n^3), kappa_n = 2 pi n / length -- the sign convention
    of etd1d_tables continued: KdV u_t + u u_x + u_xxx = 0 is c3 = +1, advection u_t + a u_x = ... is c1 = -a.  The six
    coefficient tables are complex, float32 [2, kp] host tensors (real plane, imaginary plane; padding zero), g is
    float32 [kp] as in etd1d_tables; formed in float64 / complex128 and rounded once.  Im l_{N/2} = 0: an odd derivative
    of the Nyquist mode vanishes on the grid, and with it the Nyquist bin of a real field stays real.  z = dt l_n is
    complex, so the contour is the full circle, LR = z + r_m, r_m = exp(2 pi i (m - 1/2) / 64), m = 1 .. 64, and the mean is
    the complex mean (the upper half circle with Re<.> of etd1d_tables is that mean for real z only); where z is real the
    mean is real and its imaginary part is stored as zero.  include/rpde.h has the formulas."""
    z, coefficients, g = _etd1d_tables("etd1d_tables_cx", N, length, dt, _cx_symbol(c1, c2, c3, c4), advect, dealias, True)
    return tuple(_cx_padded(z, t) for t in coefficients) + (g,)


def grf1d(noise: torch.Tensor, sqrt_eig: torch.Tensor) -> torch.Tensor:
    """noise [B, N, 2] (real and imaginary part of the coefficients in fft order, standard normal), sqrt_eig [N] ->
    [B, N] = Re ifft(sqrt_eig . noise), torch's 1/N included.  The HIP side is deterministic given the noise.
    Contiguous fp32 tensors on the GPU; no autograd, no CPU fallback."""
    return _grf("grf1d", 1, noise, sqrt_eig)


def etd1d_solve(u0: torch.Tensor, tables, steps: int, record_every: int) -> torch.Tensor:
    """`steps` ETDRK4 steps of u_t = L u - (c/2) (u^2)_x from u0 [B, N] with the seven tables of etd1d_tables ([kp]) or
    of etd1d_tables_cx (six [2, kp] and g [kp]: a symbol with odd derivatives, rpde_etd1d_steps_cx), host or device
    tensors; a snapshot -- irfft of the state -- after every `record_every`-th step.  Returns
    [B, steps // record_every, N], contiguous fp32.  Sixteen launches per step, no host synchronisation between them;
    the recording loop calls the device `steps // record_every` times, which gives the bits of one long call.
    Contiguous fp32 tensors on the GPU; no autograd, no CPU fallback."""
    lib = load()
    steps, record_every = _schedule("etd1d_solve", steps, record_every)
    u0 = _f32c(u0.detach())
    B, N = _grid(u0, "etd1d_solve", 1)
    kp = _kp(N)
    tables = tuple(tables)
    shapes = [tuple(t.shape) for t in tables]
    if shapes == [(kp,)] * 7:
        name = "etd1d_steps"
    elif shapes == [(2, kp)] * 6 + [(kp,)]:
        name = "etd1d_steps_cx"
    else:
        raise ValueError(f"etd1d_solve: expected the seven [{kp}] tables of etd1d_tables(N={N}, ...) or the six [2, {kp}] "
                         f"tables and g [{kp}] of etd1d_tables_cx(N={N}, ...)")
    pu = ptr(u0)                                           # raises for CPU tensors: there is no fallback
    dev = u0.device
    tabs = [_f32c(t.detach().to(dev)) for t in tables]
    nws = lib.rpde_etd1d_ws_bytes(B, N)
    ws = workspace(nws, dev)
    st = stream_ptr()
    U = torch.empty(lib.rpde_etd1d_spec_elems(B, N), dtype=torch.float32, device=dev)
    check(lib.rpde_etd1d_rfft(pu, ptr(U), B, N, st), "etd1d_rfft")
    n_rec = steps // record_every
    snaps = torch.empty(max(n_rec, 1), B, N, dtype=torch.float32, device=dev)
    for c in range(n_rec):
        run(name, nws, ws, ptr(U), *(ptr(t) for t in tabs), B, N, record_every)
        check(lib.rpde_etd1d_irfft(ptr(U), ptr(snaps[c]), B, N, st), "etd1d_irfft")
    return snaps[:n_rec].permute(1, 0, 2).contiguous()


# ----------------------------------------------------------------------------
# equation-residual loss of the 1-D ETD family (csrc/etd_residual.hip, rpde_etd_residual_*; utils/loss.py
# EquationResidualLoss).  Forward and backward on the device, GPU tensors only, no CPU fallback.  The Function and the
# checks of fields, tables and affine serve the 2-D vorticity residual below as well.
# ----------------------------------------------------------------------------
def etd1d_residual_tables(N: int, length: float, c1: float, c2: float, c3: float, c4: float, interval: float,
                          advect: float = 1.0, dealias: bool = True):
    """(E, m0, m1): the tables of the equation residual of u_t = L u - (advect/2) (u^2)_x over the time `interval` between
    an input and a prediction, for the symbol and g of etd1d_tables_cx, as float32 [2, kp] host tensors (real plane,
    imaginary plane; padding zero), formed in float64 / complex128 and rounded once.  With z = interval l_n, LR = z + r_m on
    the full circle's 64 points and <.> the complex mean:
        E = e^z,  m0 = interval (phi1 - phi2) i g,  m1 = interval phi2 i g,
        phi1 = <(e^LR - 1) / LR>,  phi2 = <(e^LR - 1 - LR) / LR^2>
    -- the exponential trapezoidal rule (ETD2).  The tables are always complex (i g is); where z is real the imaginary part
    of E is stored as zero, and g_0 = g_{N/2} = 0 makes m0 = m1 = 0 there.  include/rpde.h has the formulas."""
    z, LR, mean, g = _etd1d_contour("etd1d_residual_tables", N, length, interval, _cx_symbol(c1, c2, c3, c4), advect,
                                    dealias, True)
    h = float(interval)
    eLR = torch.exp(LR)
    phi1 = mean((eLR - 1.0) / LR)
    phi2 = mean((eLR - 1.0 - LR) / LR ** 2)
    # real z: the means are real, and what their imaginary parts hold is the sum's rounding, dropped before i g turns
    # it into a real part
    real = z.imag == 0
    phi1 = torch.complex(phi1.real, torch.where(real, torch.zeros_like(phi1.imag), phi1.imag))
    phi2 = torch.complex(phi2.real, torch.where(real, torch.zeros_like(phi2.imag), phi2.imag))
    ig = torch.complex(torch.zeros_like(g), g)
    m0, m1 = h * (phi1 - phi2) * ig + 0.0, h * phi2 * ig + 0.0                # + 0.0: no negative zeros where g = 0
    return (_cx_padded(z, torch.exp(z)), _padded(torch.stack([m0.real, m0.imag])), _padded(torch.stack([m1.real, m1.imag])))


def _residual_affine(affine):
    """(a_p, b_p, a_x, b_x) as a ctypes float[4], or None for the identity"""
    if affine is None:
        return None
    vals = tuple(float(v) for v in affine)
    if len(vals) != 4 or not all(v == v and abs(v) != float("inf") for v in vals):
        raise ValueError(f"etd1d_residual: affine must be four finite numbers (a_p, b_p, a_x, b_x), got {affine}")
    return (C.c_float * 4)(*vals)


class _Equation(NamedTuple):
    """What tells one equation residual from the other at the C ABI"""
    op: str                           # the op's name, for messages
    stem: str                         # the entries are rpde_<stem>_{spec_elems, fwd, bwd}
    nd: int                           # the rank of the grid
    bwd_tables: slice                 # which of the forward's tables the backward gets
    bwd_pred: bool                    # whether the backward gets the prediction
    limits: str                       # the sizes the entries serve, for the refusal of any other
    bwd_input: bool = False           # whether the backward gets the network's input
    query: str = ""                   # the size query rpde_<query>_ws_bytes, where it is not the stem's own; a name
                                      # that ends in _bytes is the whole query rpde_<query>
    square: bool = False              # the entries' dims are (B, s) of a square grid, else (B, *grid)
    table_shapes: Optional[Callable] = None       # grid -> the shape of each table; None: nd + 2 half-spectrum tables
    channels: int = 1                 # the fields are [B, channels, *grid]; one channel may be left out of the shape


_ETD1D = _Equation("etd1d_residual", "etd_residual", 1, slice(2, 3), True,
                   "N even, 4 .. 4096; 1 <= B <= 16383: four fields of B images are one batch of the half-spectrum layer")
_NS2D = _Equation("ns2d_residual", "ns2d_residual", 2, slice(2, 4), False,
                  "even axes 4 .. 4096; 8 B <= 65535 and 32 B max(M, N) < 2^31: eight derivative fields per sample are one "
                  "batch of the half-spectrum layer")
# steady, and the input is the operator's coefficient: the backward applies the operator again and needs it
_DARCY2D = _Equation("darcy2d_residual", "darcy2d_residual", 2, slice(1, 2), False,
                     "a square grid, s a multiple of 4, 8 .. 512, 1 <= B <= 65535", bwd_input=True, query="darcy2d",
                     square=True, table_shapes=lambda grid: [tuple(grid)] * 3)
# the data are (c, q, v), the equation evolves (curl u, c): three channels, seven tables (four of one diffusivity, three
# of the other).  The size query is not called *_ws_bytes (include/rpde.h has the reason)
_NSC2D = _Equation("nsc2d_residual", "nsc2d_residual", 2, slice(6, 10), False,
                   "even axes 4 .. 4096; 12 B <= 65535 and 48 B max(M, N) < 2^31: twelve derivative fields per sample are "
                   "one batch of the half-spectrum layer", query="nsc2d_residual_arena_bytes",
                   table_shapes=lambda grid: [(grid[0], _kp(grid[1]))] * 7, channels=3)


class _EquationResidual(torch.autograd.Function):
    """rpde_<stem>_fwd(p, x, *tables, affine, rel, loss, stats, spec, *dims, size_average) and
    rpde_<stem>_bwd([p,] [x,] spec, *bwd_tables, affine, stats, grad_loss, grad_rel, grad_p, *dims, size_average);
    `tables` are device tensors, None (no forcing; the L2 norm) or host floats (passed by value), checked by the caller;
    of the backward's tables the tensors come first, then the floats"""

    @staticmethod
    def forward(ctx, eq: _Equation, pred, x, tables, aff, size_average: bool, reduction: bool):
        op, stem, nd, bwd_tables, bwd_pred, limits, bwd_input, query, square, _, channels = eq   # one unpack
        lib = load()
        shape = tuple(pred.shape)
        dims = (shape[0], shape[-1]) if square else (shape[0], *shape[-nd:])
        field = (shape[0], *((channels,) if channels > 1 else ()), *shape[-nd:])
        p, x = _f32c(pred).reshape(*field), _f32c(x.detach()).reshape(*field)
        pp, px = ptr(p), ptr(x)                               # raises for CPU tensors: there is no fallback
        dev = p.device
        nws = getattr(lib, f"rpde_{query}" if query.endswith("_bytes") else f"rpde_{query or stem}_ws_bytes")(*dims)
        if nws == 0:
            sizes = " ".join(f"{n}={v}" for n, v in zip("Bs" if square else "BMN" if nd == 2 else "BN", dims))
            raise ValueError(f"{op}: unsupported {sizes} ({limits})")
        stats, rel, loss = _rel_outputs(dims[0], dev, reduction)
        spec = torch.empty(getattr(lib, f"rpde_{stem}_spec_elems")(*dims), dtype=torch.float32, device=dev)
        # ptr() is for tensors that come from outside; what was allocated here needs no check
        run(stem + "_fwd", nws, dev, pp, px, *[t if isinstance(t, float) else ptr(t) for t in tables], aff, rel.data_ptr(),
            ptr(loss), stats.data_ptr(), spec.data_ptr(), *dims, int(size_average))
        lead = ((p,) if bwd_pred else ()) + ((x,) if bwd_input else ()) + (spec,)
        kept = tables[bwd_tables]
        ctx.save_for_backward(*lead, *[t for t in kept if not isinstance(t, float)], stats)
        ctx.meta = (stem + "_bwd", shape, dims, nws, aff, size_average, reduction, [t for t in kept if isinstance(t, float)])
        return loss if reduction else rel

    @staticmethod
    def backward(ctx, g):
        *lead, stats = ctx.saved_tensors                      # ([p,] [x,] spec, the backward's tables), stats
        entry, shape, dims, nws, aff, size_average, reduction, floats = ctx.meta
        g = _f32c(g)
        gp = torch.empty(shape, dtype=torch.float32, device=stats.device)
        run(entry, nws, stats.device, *[ptr(t) for t in lead], *floats, aff, ptr(stats), *_upstream(g, reduction), gp.data_ptr(),
            *dims, int(size_average))
        return None, gp, None, None, None, None, None


def _residual_fields(eq: _Equation, pred, x, xname: str):
    """ValueError unless pred and x are equal float32 [B, *grid] or [B, 1, *grid] fields; -> the grid.  A CPU tensor
    gets as far as the Function's ptr(): the CPU refusal of every op"""
    nd, shape, d = eq.nd, pred.shape, pred.dim()
    if shape != x.shape or not (d == nd + 1 or (d == nd + 2 and shape[1] == 1)):
        grid = "N" if nd == 1 else "M, N"
        raise ValueError(f"{eq.op}: pred {tuple(shape)} / {xname} {tuple(x.shape)}, expected equal [B, {grid}] or "
                         f"[B, 1, {grid}] shapes (one channel)")
    if pred.dtype != torch.float32 or x.dtype != torch.float32:
        raise ValueError(f"{eq.op}: expected float32 fields, got {pred.dtype} / {x.dtype}")
    return shape[-nd:]


def _residual_tables(eq: _Equation, tables, grid, device):
    """ValueError unless `tables` are the three [2, kp] (1-D) or four [M, kp] (2-D) tables of <op>_tables for this grid;
    -> the tables, detached, as contiguous fp32 tensors on the device"""
    tables = tuple(tables)
    if eq.table_shapes is not None:
        # tables of shapes of the equation's own; None stands for a table the chosen variant does not take
        shapes = eq.table_shapes(grid)
        if len(tables) != len(shapes) or any(t is not None and (not torch.is_tensor(t) or tuple(t.shape) != sh)
                                             for t, sh in zip(tables, shapes)):
            sizes = ", ".join(f"{n}={v}" for n, v in zip("MN"[-eq.nd:], grid))
            raise ValueError(f"{eq.op}: expected the {len(shapes)} tables {[list(sh) for sh in shapes]} of "
                             f"{eq.op}_tables({sizes}, ...), got "
                             f"{[tuple(t.shape) if torch.is_tensor(t) else t for t in tables]}")
        return tuple(None if t is None else _f32c(t.detach().to(device)) for t in tables)
    count, shape = eq.nd + 2, (2 if eq.nd == 1 else grid[0], _kp(grid[-1]))
    if len(tables) != count or any(tuple(t.shape) != shape for t in tables):
        sizes = ", ".join(f"{n}={v}" for n, v in zip("MN"[-eq.nd:], grid))
        raise ValueError(f"{eq.op}: expected the {('three', 'four')[count - 3]} {list(shape)} tables of "
                         f"{eq.op}_tables({sizes}, ...), got {[tuple(t.shape) for t in tables]}")
    return tuple(_f32c(t.detach().to(device)) for t in tables)


def etd1d_residual(pred, x, tables, affine=None, size_average: bool = True, reduction: bool = True):
    """Does pred ~ u(t + interval) follow from x = u(t) under u_t = L u - (c/2) (u^2)_x?  With the tables (E, m0, m1) of
    etd1d_residual_tables (host or device tensors, [2, kp] each),
        r^ = rfft(p~) - E rfft(x~) - m0 rfft(x~^2) - m1 rfft(p~^2),   rel[b] = |r[b]|_2 / (|x~[b]|_2 + 1e-8),
    then mean / sum / the per-sample vector as relative_l2.  affine = (a_p, b_p, a_x, b_x): p~ = a_p pred + b_p,
    x~ = a_x x + b_x (None: the identity); the gradient is with respect to pred itself.  The rule is the exponential
    trapezoidal one: exact in the linear part, second order in the nonlinear one, so the residual of an exact pair is
    O(interval^3 N_tt) and the loss is for |interval N_tt| small (DESIGN.md has the table: on KS at N = 64 an exact
    pair gives rel ~ 1e-3 at interval 0.05, ~ 1e-2 at 0.1 and ~ 1 by 0.4).  pred, x: [B, N] or [B, 1, N] (one channel:
    the equation is scalar) contiguous fp32 tensors on the GPU; gradient for pred only, no CPU fallback."""
    tables = _residual_tables(_ETD1D, tables, _residual_fields(_ETD1D, pred, x, "x"), pred.device)
    return _EquationResidual.apply(_ETD1D, pred, x, tables, _residual_affine(affine), bool(size_average), bool(reduction))


# ----------------------------------------------------------------------------
# equation-residual loss of the 2-D vorticity equation (csrc/ns_residual.hip, rpde_ns2d_residual_*; utils/loss.py
# VorticityResidualLoss).  Forward and backward on the device, GPU tensors only, no CPU fallback.
# ----------------------------------------------------------------------------
def _ns2d_residual_phi(what: str, M, N, visc, interval):
    """(z, phi1, phi2, dealias, poisson), float64 [M, K]: z = -interval visc lap on the grid of ns2d_tables and the two
    phi functions of the exponential trapezoidal rule on the full circle's 64 contour points (z is real: so are they)"""
    import math
    M, N = int(M), int(N)
    if M < 4 or N < 4 or M % 2 or N % 2:
        raise ValueError(f"{what}: M and N must be even and >= 4, got {M} x {N}")
    if not (math.isfinite(float(visc)) and float(visc) >= 0 and math.isfinite(float(interval)) and float(interval) > 0):
        raise ValueError(f"{what}: visc must be >= 0 and interval positive, got visc={visc} interval={interval}")
    lap, dealias, poisson = _ns2d_symbols(M, N)
    z = -float(interval) * float(visc) * lap
    LR, mean = _contour(z, True)
    eLR = torch.exp(LR)
    return z, mean((eLR - 1.0) / LR).real, mean((eLR - 1.0 - LR) / LR ** 2).real, dealias, poisson


def ns2d_residual_tables(M: int, N: int, visc: float, interval: float, dealias: bool = True):
    """(em1, m0, m1, inv_lap): the tables of the equation residual of w_t = -visc lap w - A(w) + f over the time `interval`
    between an input and a prediction, on the grid and with the symbols of ns2d_tables, as float32 [M, kp] host tensors
    (padded columns zero), formed in float64 and rounded once.  With z = -interval visc lap and phi1, phi2 as in
    etd1d_residual_tables (real here):
        em1 = e^z - 1 (expm1),  m0 = interval (phi1 - phi2) dealias,  m1 = interval phi2 dealias,  inv_lap = 1 / lap
    (the mean mode's lap set to 1 for the division).  dealias=False drops the 2/3 mask.  include/rpde.h has the formulas."""
    z, phi1, phi2, keep, poisson = _ns2d_residual_phi("ns2d_residual_tables", M, N, visc, interval)
    if not dealias:
        keep = torch.ones_like(keep)
    h = float(interval)
    return tuple(_padded(t) for t in (torch.expm1(z), h * (phi1 - phi2) * keep, h * phi2 * keep, 1.0 / poisson))


def ns2d_residual_forcing(f: torch.Tensor, visc: float, interval: float) -> torch.Tensor:
    """The forcing term of the residual, (m0 + m1) rfft2(f) = interval phi1 rfft2(f), for one forcing field f [M, N]: a
    float32 [M, 2, kp] host tensor (real plane, imaginary plane; padded columns zero), formed in float64 and rounded once.
    Not de-aliased: the generator adds its forcing as it stands."""
    if f.dim() != 2:
        raise ValueError(f"ns2d_residual_forcing: forcing {tuple(f.shape)}, expected [M, N] (one field for the batch)")
    M, N = (int(v) for v in f.shape)
    _, phi1, _, _, _ = _ns2d_residual_phi("ns2d_residual_forcing", M, N, visc, interval)
    s = float(interval) * phi1 * torch.fft.rfft2(f.detach().double().cpu())
    return _padded(torch.stack([s.real, s.imag], dim=1)).contiguous()


def ns2d_residual_spectrum(x: torch.Tensor, affine=None):
    """(spec64, spec32): rfft2 of a x + b for x [B, M, N] by the float64 analysis of the residual's forward (rows, then
    columns, float64 sums), as [B, M, 2, kp] float64 and its fp32 rounding.  affine = (a, b) or None.  GPU tensors only."""
    lib = load()
    x = _f32c(x.detach())
    px = ptr(x)
    if x.dim() != 3:
        raise ValueError(f"ns2d_residual_spectrum: expected [B, M, N], got {tuple(x.shape)}")
    B, M, N = (int(v) for v in x.shape)
    nws = lib.rpde_ns2d_residual_ws_bytes(B, M, N)
    if nws == 0:
        raise ValueError(f"ns2d_residual_spectrum: unsupported B={B} M={M} N={N} (even axes 4 .. 4096, 8 B <= 65535)")
    s64 = torch.empty(B, M, 2, _kp(N), dtype=torch.float64, device=x.device)
    s32 = torch.empty(B, M, 2, _kp(N), dtype=torch.float32, device=x.device)
    aff = None if affine is None else (C.c_float * 2)(float(affine[0]), float(affine[1]))
    run("ns2d_residual_spectrum", nws, x.device, px, aff, s64.data_ptr(), ptr(s32), B, M, N)
    return s64, s32


def ns2d_residual(pred, inp, tables, forcing_spec=None, affine=None, size_average: bool = True, reduction: bool = True):
    """Does pred ~ w(t + interval) follow from inp = w(t) under the vorticity equation of the generator (ns2d_solve),
    w_t = -visc lap w - A(w) + f?  With the tables (em1, m0, m1, inv_lap) of ns2d_residual_tables (host or device tensors,
    [M, kp] each) and forcing_spec of ns2d_residual_forcing ([M, 2, kp], or None: no forcing),
        r^ = rfft2(p~ - x~) - em1 rfft2(x~) - forcing_spec + m0 rfft2(N(x~)) + m1 rfft2(N(p~)),  N(w) = q w_x + v w_y,
        rel[b] = |r[b]|_2 / (|x~[b]|_2 + 1e-8),
    then mean / sum / the per-sample vector as relative_l2.  affine = (a_p, b_p, a_x, b_x): p~ = a_p pred + b_p,
    x~ = a_x inp + b_x (None: the identity); the gradient is with respect to pred itself.  The rule is the exponential
    trapezoidal one, second order in the nonlinear term: the loss is for |interval N_tt| small (DESIGN.md 10.12 has the
    table).  pred, inp: [B, M, N] or [B, 1, M, N] (one channel: the vorticity is scalar) contiguous fp32 tensors on the
    GPU; gradient for pred only, no CPU fallback."""
    M, N = grid = _residual_fields(_NS2D, pred, inp, "inp")
    tables = _residual_tables(_NS2D, tables, grid, pred.device)
    if forcing_spec is not None and tuple(forcing_spec.shape) != (M, 2, _kp(N)):
        raise ValueError(f"ns2d_residual: forcing_spec {tuple(forcing_spec.shape)}, expected the [{M}, 2, {_kp(N)}] spectrum of "
                         "ns2d_residual_forcing")
    fs = None if forcing_spec is None else _f32c(forcing_spec.detach().to(pred.device))
    return _EquationResidual.apply(_NS2D, pred, inp, tables + (fs,), _residual_affine(affine), bool(size_average),
                                   bool(reduction))


# ----------------------------------------------------------------------------
# equation-residual loss of the active-scalar system (csrc/nsc_residual.hip, rpde_nsc2d_residual_*; utils/loss.py
# ActiveScalarResidualLoss).  Forward and backward on the device, GPU tensors only, no CPU fallback.
# ----------------------------------------------------------------------------
def nsc2d_residual_tables(M: int, N: int, visc: float, kappa: float, interval: float):
    """(em1_nu, m0_nu, m1_nu, inv_lap, em1_kappa, m0_kappa, m1_kappa): ns2d_residual_tables once with the viscosity and
    once with the scalar's diffusivity (z = -interval kappa lap), float32 [M, kp] host tensors, padded columns zero."""
    return ns2d_residual_tables(M, N, visc, interval) + ns2d_residual_tables(M, N, kappa, interval)[:3]


def nsc2d_residual(pred, inp, tables, beta: float, forcing_spec=None, scalar_weight: float = 1.0, affine=None,
                   size_average: bool = True, reduction: bool = True):
    """Does pred ~ (c, q, v)(t + interval) follow from inp = (c, q, v)(t) under the active-scalar system of the generator
    (nsc2d_solve): w_t + u . grad w = visc lap w + beta dc/dx1 + f, c_t + u . grad c = kappa lap c, w = curl u?  With the
    seven tables of nsc2d_residual_tables (host or device tensors, [M, kp] each), forcing_spec of ns2d_residual_forcing at
    the viscosity ([M, 2, kp], or None: no forcing), X_w = 2 pi i k1 x^_v - 2 pi i k2 x^_q, X_c = x^_c, likewise D from
    d = p~ - x~, P = X + D, and the generator's N_w (advection and buoyancy) and N_c,
        r^_w = D_w - em1_nu X_w + m0_nu N_w(X) + m1_nu N_w(P) - forcing_spec,   r^_c = D_c - em1_kappa X_c + m0_kappa N_c(X)
        + m1_kappa N_c(P),   delta^ = 2 pi i (k1 P_q + k2 P_v),   mu = the change of the mean of (q, v),
        E_ru = sum_{k != 0} c (|r^_w|^2 + |delta^|^2) / lap / (M N) + |mu|^2 / (M N),   E_rc = sum c |r^_c|^2 / (M N),
        rel[b] = sqrt(scalar_weight E_rc + E_ru) / (sqrt(scalar_weight |x~_c|^2 + |x~_q|^2 + |x~_v|^2) + 1e-8),
    then mean / sum / the per-sample vector as relative_l2: the vorticity's residual measured as a velocity, next to
    what the predicted velocity owes to incompressibility and to its mean.  affine = (a_p, b_p, a_x, b_x), one map for
    the three channels: p~ = a_p pred + b_p, x~ = a_x inp + b_x (None: the identity); the gradient is with respect to
    pred itself.  The rule is the exponential trapezoidal one (DESIGN.md 10.15 has the range of validity).  pred, inp:
    [B, 3, M, N] = (c, q, v) contiguous fp32 tensors on the GPU; gradient for pred only, no CPU fallback."""
    import math
    eq = _NSC2D
    if pred.shape != inp.shape or pred.dim() != 4 or pred.shape[1] != 3:
        raise ValueError(f"{eq.op}: pred {tuple(pred.shape)} / inp {tuple(inp.shape)}, expected equal [B, 3, M, N] shapes: "
                         "the three channels (c, q, v), concentration and velocity")
    if pred.dtype != torch.float32 or inp.dtype != torch.float32:
        raise ValueError(f"{eq.op}: expected float32 fields, got {pred.dtype} / {inp.dtype}")
    M, N = grid = tuple(int(n) for n in pred.shape[-2:])
    beta, lam = float(beta), float(scalar_weight)
    if not (math.isfinite(beta) and math.isfinite(lam) and lam >= 0.0):
        raise ValueError(f"{eq.op}: beta {beta} must be finite and scalar_weight {scalar_weight} finite and >= 0")
    em1n, m0n, m1n, il, em1k, m0k, m1k = _residual_tables(eq, tables, grid, pred.device)
    if forcing_spec is not None and tuple(forcing_spec.shape) != (M, 2, _kp(N)):
        raise ValueError(f"{eq.op}: forcing_spec {tuple(forcing_spec.shape)}, expected the [{M}, 2, {_kp(N)}] spectrum of "
                         "ns2d_residual_forcing")
    fs = None if forcing_spec is None else _f32c(forcing_spec.detach().to(pred.device))
    # the forward's own tables, then what the backward takes as well (m1_nu, m1_kappa, inv_lap, beta)
    return _EquationResidual.apply(eq, pred, inp, (em1n, m0n, em1k, m0k, fs, lam, m1n, m1k, il, beta),
                                   _residual_affine(affine), bool(size_average), bool(reduction))


def nsc2d_residual_state(pred, inp, affine=None):
    """[4, B, M, 2, kp] = (X_w, P_w, X_c, P_c): the state the residual's forward hands to the generator's fan-out -- the
    curl of the velocity channels and the scalar, of x~ and of p~ = x~ + d -- from the float64 analysis, rounded once.
    pred, inp [B, 3, M, N]; affine as nsc2d_residual.  GPU tensors only."""
    lib = load()
    p, x = _f32c(pred.detach()), _f32c(inp.detach())
    pp, px = ptr(p), ptr(x)
    if p.shape != x.shape or p.dim() != 4 or p.shape[1] != 3:
        raise ValueError(f"nsc2d_residual_state: expected equal [B, 3, M, N] fields (c, q, v), got {tuple(p.shape)} / {tuple(x.shape)}")
    B, _, M, N = (int(v) for v in p.shape)
    nws = lib.rpde_nsc2d_residual_arena_bytes(B, M, N)
    if nws == 0:
        raise ValueError(f"nsc2d_residual_state: unsupported B={B} M={M} N={N} ({_NSC2D.limits})")
    out = torch.empty(4, B, M, 2, _kp(N), dtype=torch.float32, device=p.device)
    run("nsc2d_residual_state", nws, p.device, pp, px, _residual_affine(affine), ptr(out), B, M, N)
    return out


# ----------------------------------------------------------------------------
# Darcy flow generator (csrc/darcy.hip, rpde_darcy2d_* / rpde_sep2d; data_generation/darcy_2d.py and
# random_fields.py GaussianRFNeumann are the callers).  Data production: no autograd, GPU tensors only, no CPU fallback.
# ----------------------------------------------------------------------------
def _darcy_grid(t: torch.Tensor, what: str):
    """(B, s) of a batch of square fields [B, s, s], refused as the C side refuses them"""
    if t.dim() != 3 or t.shape[1] != t.shape[2]:
        raise ValueError(f"{what}: expected [B, s, s], got {tuple(t.shape)}")
    B, s = int(t.shape[0]), int(t.shape[1])
    if load().rpde_darcy2d_ws_bytes(B, s) == 0:
        raise ValueError(f"{what}: unsupported grid B={B} s={s} (s a multiple of 4, 8 .. 512, 1 <= B <= 65535)")
    return B, s


def darcy2d_tables(s: int):
    """(S, inv_lambda): float32 [s, s] host tensors, formed in float64 and rounded once.
    S[k, i] = sqrt(2/s) sin(pi (k+1) (i+1/2) / s) with row s-1 divided by sqrt 2 (DST-II, orthogonal);
    inv_lambda[k1, k2] = 1 / (l_k1 + l_k2), l_k = s^2 (2 - 2 cos(pi (k+1) / s)): the eigenvalues of the finite-volume
    Dirichlet Laplacian on cell centres, whose eigenvectors are the rows of S."""
    S, inv_lambda = _darcy2d_tables64("darcy2d_tables", s)
    return S.to(torch.float32), inv_lambda.to(torch.float32)


def _darcy2d_tables64(what: str, s):
    """(S, inv_lambda) of darcy2d_tables in float64, before the rounding"""
    import math
    s = int(s)
    if s < 8 or s > 512 or s % 4:
        raise ValueError(f"{what}: s must be a multiple of 4, 8 .. 512, got {s}")
    k = torch.arange(1, s + 1, dtype=torch.float64).view(s, 1)
    x = (torch.arange(s, dtype=torch.float64) + 0.5).view(1, s)
    S = math.sqrt(2.0 / s) * torch.sin(math.pi * k * x / s)
    S[s - 1] /= math.sqrt(2.0)
    lam = float(s) ** 2 * (2.0 - 2.0 * torch.cos(math.pi * k.view(-1) / s))
    return S, 1.0 / (lam.view(s, 1) + lam.view(1, s))


def sep2d(x: torch.Tensor, L: torch.Tensor, R: torch.Tensor) -> torch.Tensor:
    """out[b] = L x[b] R^T for x [B, s, s] and two tables [s, s]: a separable transform as two matrix products.
    Contiguous fp32 tensors on the GPU; no autograd, no CPU fallback."""
    lib = load()
    x, L, R = _f32c(x.detach()), _f32c(L.detach()), _f32c(R.detach())
    px, pl, pr = ptr(x), ptr(L), ptr(R)                    # raises for CPU tensors: there is no fallback
    B, s = _darcy_grid(x, "sep2d")
    if tuple(L.shape) != (s, s) or tuple(R.shape) != (s, s):
        raise ValueError(f"sep2d: tables {tuple(L.shape)} and {tuple(R.shape)}, expected {(s, s)}")
    out = torch.empty_like(x)
    run("sep2d", B * s * s * 4 + 256, x.device, px, pl, pr, ptr(out), B, s)
    return out


def darcy2d_apply(a: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """A u for the finite-volume operator of -div(a grad .) with u = 0 on the boundary (include/rpde.h has the
    formulas): a, u [B, s, s] at the cell centres.  Contiguous fp32 tensors on the GPU; no autograd, no CPU fallback."""
    lib = load()
    a, u = _f32c(a.detach()), _f32c(u.detach())
    pa, pu = ptr(a), ptr(u)                                # raises for CPU tensors: there is no fallback
    B, s = _darcy_grid(a, "darcy2d_apply")
    if tuple(u.shape) != (B, s, s):
        raise ValueError(f"darcy2d_apply: u {tuple(u.shape)}, expected {(B, s, s)}")
    out = torch.empty_like(u)
    check(lib.rpde_darcy2d_apply(pa, pu, ptr(out), B, s, stream_ptr()), "darcy2d_apply")
    return out


def darcy2d_solve(a: torch.Tensor, f: torch.Tensor, iterations: int = 24, tol: float = 1e-6):
    """-div(a grad u) = f on the unit square with u = 0 on the boundary, finite volumes on the s x s cell centres:
    `iterations` iterations of conjugate gradients preconditioned with the constant-coefficient operator (two sine
    transforms as matrix products).  a [B, s, s] positive and finite (checked here: one device-to-host read before the
    solve, none inside it), f [s, s] for the whole batch or [B, s, s].  Returns (u [B, s, s], rel_residual [B] =
    |f - A u| / |f| recomputed after the loop, frozen_at [B] int32 = the iterations a sample took until |r| <= tol |f|,
    `iterations` if it never got there).  Nine launches per iteration; identical calls give identical bits.  Contiguous
    fp32 tensors on the GPU; no autograd, no CPU fallback."""
    import math
    lib = load()
    iterations, tol = int(iterations), float(tol)
    if iterations < 0 or not (tol >= 0.0 and math.isfinite(tol)):
        raise ValueError(f"darcy2d_solve: bad iterations={iterations} tol={tol}")
    a, f = _f32c(a.detach()), _f32c(f.detach())
    pa, pf = ptr(a), ptr(f)                                # raises for CPU tensors: there is no fallback
    B, s = _darcy_grid(a, "darcy2d_solve")
    if tuple(f.shape) not in ((s, s), (B, s, s)):
        raise ValueError(f"darcy2d_solve: right-hand side {tuple(f.shape)}, expected {(s, s)} or {(B, s, s)}")
    if not bool((torch.isfinite(a) & (a > 0)).all()):
        raise ValueError("darcy2d_solve: the coefficient a must be positive and finite everywhere")
    dev = a.device
    S, inv_lambda = (t.to(dev) for t in darcy2d_tables(s))
    u = torch.empty_like(a)
    rel = torch.empty(B, dtype=torch.float32, device=dev)
    frozen_at = torch.empty(B, dtype=torch.int32, device=dev)
    run("darcy2d_solve", lib.rpde_darcy2d_ws_bytes(B, s), dev, pa, pf, int(f.dim() == 3), ptr(S), ptr(inv_lambda),
        ptr(u), ptr(rel), frozen_at.data_ptr(), B, s, iterations, tol)
    return u, rel, frozen_at


# ----------------------------------------------------------------------------
# equation-residual loss of the Darcy generator (csrc/darcy_residual.hip, rpde_darcy2d_residual_*; utils/loss.py
# DarcyResidualLoss).  Forward and backward on the device, GPU tensors only, no CPU fallback.
# ----------------------------------------------------------------------------
DARCY_NORMS = ("dual", "l2")


def darcy2d_residual_tables(s: int, forcing=1.0, norm: str = "dual"):
    """(f, S, inv_lambda, D): what the Darcy equation residual needs on an s x s grid.  f: the right-hand side, float32
    [s, s] on the host -- a constant (the generator's --forcing) or one [s, s] field, rounded once.  norm="dual": S and
    inv_lambda of darcy2d_tables and D = sqrt(sum_k inv_lambda_k (S f S^T)_k^2), the norm of f that the preconditioner
    P = A(1) induces (f . P^-1 f); norm="l2": S = inv_lambda = None and D = |f|_2.  D is a Python float, formed in
    float64 from the rounded f and the unrounded tables.  f = 0 is a ValueError: the ratio has no denominator."""
    import math
    if norm not in DARCY_NORMS:
        raise ValueError(f"darcy2d_residual_tables: norm must be one of {DARCY_NORMS}, got {norm!r}")
    S, inv_lambda = _darcy2d_tables64("darcy2d_residual_tables", s)
    s = int(s)
    if torch.is_tensor(forcing):
        if tuple(forcing.shape) != (s, s):
            raise ValueError(f"darcy2d_residual_tables: forcing {tuple(forcing.shape)}, expected one [{s}, {s}] field for "
                             "the batch")
        f = forcing.detach().cpu().to(torch.float32).contiguous()
    else:
        f = torch.full((s, s), float(forcing), dtype=torch.float32)
    f64 = f.double()
    if not bool(torch.isfinite(f64).all()):
        raise ValueError("darcy2d_residual_tables: the forcing must be finite")
    if norm == "dual":
        D = math.sqrt(float((inv_lambda * (S @ f64 @ S.T) ** 2).sum()))
    else:
        D = math.sqrt(float((f64 ** 2).sum()))
    if not D > 0.0:
        raise ValueError("darcy2d_residual_tables: the forcing is zero: the relative residual has no denominator")
    if norm == "l2":
        return f, None, None, D
    return f, S.to(torch.float32), inv_lambda.to(torch.float32), D


def darcy2d_residual(pred, a, tables, affine=None, size_average: bool = True, reduction: bool = True):
    """Does pred ~ u solve -div(a grad u) = f, u = 0 on the boundary, in the discretisation of the generator
    (darcy2d_solve)?  With the tables (f, S, inv_lambda, D) of darcy2d_residual_tables (host or device tensors) and
    r = f - A(a~) p~, A the operator of darcy2d_apply,
        norm="dual":  rel[b] = sqrt(sum_k inv_lambda_k (S r[b] S^T)_k^2) / (D + 1e-8)   (r . P^-1 r, P = A(1))
        norm="l2":    rel[b] = |r[b]|_2 / (D + 1e-8)                                   (S = inv_lambda = None)
    then mean / sum / the per-sample vector as relative_l2.  affine = (a_p, b_p, a_x, b_x): p~ = a_p pred + b_p,
    a~ = a_x a + b_x (None: the identity); the gradient is with respect to pred itself.  The dual norm is the
    energy-norm error of the prediction to within sqrt(a_max / a_min), whatever the grid; the L2 form grows like s^2
    (DESIGN.md 10.14).  A decoded coefficient that is not positive makes the loss non-finite (not checked: the
    optimizer's non-finite step skipping takes such a step).  pred, a: [B, s, s] or [B, 1, s, s] contiguous fp32
    tensors on the GPU, s a multiple of 4 in 8 .. 512; gradient for pred only, no CPU fallback."""
    eq = _DARCY2D
    grid = tuple(int(n) for n in _residual_fields(eq, pred, a, "a"))
    if grid[0] != grid[1] or grid[0] < 8 or grid[0] > 512 or grid[0] % 4:
        raise ValueError(f"{eq.op}: unsupported grid {grid} ({eq.limits})")
    tables = tuple(tables)
    if len(tables) != 4 or isinstance(tables[3], bool) or not isinstance(tables[3], (int, float)) or \
            (tables[1] is None) != (tables[2] is None) or tables[0] is None:
        raise ValueError(f"{eq.op}: expected the tables (f, S, inv_lambda, D) of darcy2d_residual_tables(s={grid[0]}, ...)")
    D = float(tables[3])
    if not (D > 0.0 and D < float("inf")):
        raise ValueError(f"{eq.op}: the norm D of the right-hand side must be positive and finite, got {D}")
    fields = _residual_tables(eq, tables[:3], grid, pred.device)
    return _EquationResidual.apply(eq, pred, a, fields + (D,), _residual_affine(affine), bool(size_average), bool(reduction))


# ----------------------------------------------------------------------------
# CNO: resampling tables and the fused alias-free activation (rpde/cno.py)
# ----------------------------------------------------------------------------
from .cno import (CnoBand, CnoTables, batchnorm1d, batchnorm2d, cno_act1d, cno_act2d, cno_dense,  # noqa: E402,F401
                  cno_resample_table, cno_tables, cno_transpose_band, conv1d_k3, conv2d_k3, skip_add)

# ----------------------------------------------------------------------------
# U-Net: norm -> tanh (-> MaxPool) in one pass, ConvTranspose(k = 2, stride = 2) (rpde/unet.py)
# ----------------------------------------------------------------------------
from .unet import groupnorm_tanh, norm_tanh, tanh_pool, upconv1d, upconv2d  # noqa: E402,F401


def warm_plans(model, resolutions, dims: int, in_channels: int = 1, device="cuda") -> None:
    """Build every DFT plan (tables, adjoint tables, operand images: hipMalloc + one stream sync each,
    csrc/core.hip get_plan) and size the workspaces the model needs at the given grid resolutions, with one
    throw-away forward per resolution -- so that no allocation or synchronisation happens inside a training
    step, and hipGraph capture never meets a first-use plan.  Leaves parameters and the train/eval flag alone."""
    was_training = model.training
    model.eval()
    with torch.no_grad():
        for r in sorted({int(r) for r in resolutions}):
            model(torch.zeros((1, in_channels) + (r,) * dims, device=device))
    model.train(was_training)
    torch.cuda.synchronize(device)
