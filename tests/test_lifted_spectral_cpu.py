"""The identity behind FFNO2D's first layer on the unlifted input (csrc/lifted_spectral.hip), in float64
torch on the CPU, against autograd of the composed reference (oracle/reference_path.py):

    forward_fourier(u W_in^T + b_in) = synthesis(mix'(analysis([u | 1])))     W'[k][j][o] = sum_i W~[i][j] Wmix[k][i][o]

and the gradients the backward forms from T[k][j][o] = sum_lines conj(S_u~[line][k][j]) G[line][k][o] alone: no adjoint
mix, no adjoint synthesis, no gradient of the lifted field.  `lifted_forward` / `lifted_grads` restate the kernels'
arithmetic (the spectrum of the constant channel is sqrt(n) at k = 0; G is the cotangent of the mixed spectrum)."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import reference_path as R

C, CIN = 64, 3


def _axis_parts(u, w_in, b_in, w_mix, K, dim):
    """spectra of [u | 1] along `dim` of the channels-first field, W~ and the complex mix weight, cut to the kept modes"""
    n = u.shape[dim]
    k = min(K, n // 2 + 1)
    s = torch.fft.rfft(u, dim=dim, norm="ortho").narrow(dim, 0, k)
    const = torch.zeros_like(s[:, :1])
    const.narrow(dim, 0, 1).fill_(math.sqrt(n))                      # analysis of the constant 1
    s = torch.cat((s, const), dim=1)
    wt = torch.cat((w_in, (b_in if b_in is not None else torch.zeros_like(w_in[:, 0])).unsqueeze(1)), dim=1)
    wc = torch.view_as_complex(w_mix[:, :, :k].contiguous())
    return n, k, s, wt, wc


def _synthesis(mixed, n, k, dim):
    shape = list(mixed.shape)
    shape[dim] = n // 2 + 1
    full = mixed.new_zeros(shape)
    full.narrow(dim, 0, k).copy_(mixed)
    return torch.fft.irfft(full, n=n, dim=dim, norm="ortho")


def lifted_forward(u, w_in, b_in, w_y, w_x, K):
    """u [B,M,N,Cin] -> forward_fourier of the lifted field, [B,M,N,C], through W' on Cin + 1 channels"""
    ut = u.permute(0, 3, 1, 2)
    out = 0
    for dim, w_mix, eq in ((-1, w_y, "bjxy,joy->boxy"), (-2, w_x, "bjxy,jox->boxy")):
        n, k, s, wt, wc = _axis_parts(ut, w_in, b_in, w_mix, K, dim)
        wp = torch.einsum("ij,iok->jok", wt.to(wc.dtype), wc)
        out = out + _synthesis(torch.einsum(eq, s, wp), n, k, dim)
    return out.permute(0, 2, 3, 1)


def lifted_grads(u, w_in, b_in, w_y, w_x, K, g):
    """(gW_in, gb_in, gw_y, gw_x) from T alone; g [B,M,N,C] is the cotangent of the branch's output"""
    ut, gt = u.permute(0, 3, 1, 2), g.permute(0, 3, 1, 2)
    gw_in = torch.zeros_like(w_in)
    gb_in = torch.zeros_like(w_in[:, 0])
    gws = []
    for dim, w_mix, eq in ((-1, w_y, "bjxy,boxy->joy"), (-2, w_x, "bjxy,boxy->jox")):
        n, k, s, wt, wc = _axis_parts(ut, w_in, b_in, w_mix, K, dim)
        # G: cotangent of the mixed spectrum = the adjoint synthesis of g (what the analysis kernel computes with the
        # transposed synthesis table), here by autograd through the synthesis only
        shape = list(gt.shape)
        shape[dim] = k
        with torch.enable_grad():
            mixed = torch.zeros(shape, dtype=wc.dtype, requires_grad=True)
            (G,) = torch.autograd.grad(_synthesis(mixed, n, k, dim), mixed, gt)
        T = torch.einsum(eq, s.conj(), G)                                    # [j][o][k]
        gw = torch.einsum("ij,jok->iok", wt.to(T.dtype), T)
        full = torch.zeros_like(w_mix)
        full[:, :, :k] = torch.view_as_real(gw)
        gws.append(full)
        gwt = torch.einsum("iok,jok->ij", wc.real, T.real) + torch.einsum("iok,jok->ij", wc.imag, T.imag)
        gw_in += gwt[:, :-1]
        gb_in += gwt[:, -1]
    return gw_in, gb_in, gws[0], gws[1]


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("K", [20, 5])
@pytest.mark.parametrize("M,N", [(32, 32), (32, 48)])
def test_lifted_identity_and_t_gradients_match_the_composed_reference(M, N, K, bias):
    torch.manual_seed(1000 * M + 10 * N + K + bias)
    B = 2
    dd = torch.float64
    u = torch.randn(B, M, N, CIN, dtype=dd)
    w_in = (torch.randn(C, CIN, dtype=dd) / math.sqrt(CIN)).requires_grad_()
    b_in = torch.randn(C, dtype=dd).requires_grad_() if bias else None
    w_y = (torch.randn(C, C, K, 2, dtype=dd) / C).requires_grad_()
    w_x = (torch.randn(C, C, K, 2, dtype=dd) / C).requires_grad_()
    g = torch.randn(B, M, N, C, dtype=dd)
    assert (min(K, N // 2 + 1) < K or min(K, M // 2 + 1) < K) == (K == 20)   # K = 20 clamps on these grids

    ref = R.fspectral2d_fourier(F.linear(u, w_in, b_in), w_y, w_x, K)
    leaves = [w_in, w_y, w_x] + ([b_in] if bias else [])
    ref_g = torch.autograd.grad(ref, leaves, g)
    with torch.no_grad():
        out = lifted_forward(u, w_in, b_in, w_y, w_x, K)
        gw_in, gb_in, gw_y, gw_x = lifted_grads(u, w_in, b_in, w_y, w_x, K, g)

    def rel(a, b):
        return float((a - b).norm() / b.norm())
    assert rel(out, ref.detach()) < 1e-13
    assert rel(gw_in, ref_g[0]) < 1e-13
    assert rel(gw_y, ref_g[1]) < 1e-13
    assert rel(gw_x, ref_g[2]) < 1e-13
    if bias:
        assert rel(gb_in, ref_g[3]) < 1e-13
    # the modes the clamp drops receive no gradient, as in the reference
    for gw, n in ((gw_y, N), (gw_x, M)):
        assert not gw[:, :, min(K, n // 2 + 1):].any()


def test_lifted_entries_carve_from_the_layer_query():
    """rpde_lifted_fspectral2d_fwd / _bwd take their workspace from rpde_fspectral2d_ws_bytes: they accept that much for
    every Cin they cover and refuse a short one before touching a device (dummy pointers: no call gets further)."""
    from rpde import _lib
    lib = _lib.load()
    fake = 1 << 20
    B, M, N, K = 2, 64, 64, 20
    need = lib.rpde_fspectral2d_ws_bytes(B, M, N, C, K)
    assert lib.rpde_lifted_fspectral2d_ok(M, N, C, 3, K) == 1
    assert lib.rpde_lifted_fspectral2d_ok(M, N, C, 5, K) == 0 and lib.rpde_lifted_fspectral2d_ok(M, N, 32, 3, K) == 0
    assert lib.rpde_lifted_fspectral2d_ok(32, 48, C, 3, K) == 0            # 20 modes clamp to 17 along one axis only
    for cin in (1, 2, 3, 4):
        assert lib.rpde_lifted_fspectral2d_spec_elems(B, M, N, cin, K) == 2 * B * 64 * 40 * cin
        for entry, nptr in (("fwd", 7), ("bwd", 10)):
            fn = getattr(lib, "rpde_lifted_fspectral2d_" + entry)
            assert fn(*([fake] * nptr), B, M, N, C, cin, K, fake, 256, None) == _lib.ERR_WORKSPACE
            msg = lib.rpde_last_error().decode()
            assert msg.startswith(f"lifted_fspectral2d_{entry}: workspace too small (256 bytes, needs "), msg
            assert int(msg.rsplit("needs ", 1)[1].rstrip(")")) <= need
