"""float64 restatement of the 2-D CNO activation and blocks (reference models/CNO2d.py), test infrastructure only.  The
per-axis resampling matrices are those of tests/cno_ref.py: F.interpolate applied to an identity, never the tables of
the code under test.  Sizes are (rows, columns) pairs."""
import torch
import torch.nn.functional as F

from tests.cno_ref import min_margin, resample_matrix  # noqa: F401  (min_margin is part of this module's interface)


def affine(x, scale, shift):
    x = x.double()
    return x if scale is None else x * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)


def resample(x, size):
    """x [B, C, H, W] float64 -> size = (h, w): R_y x R_x^T"""
    Ry, Rx = resample_matrix(x.shape[-2], size[0]), resample_matrix(x.shape[-1], size[1])
    return torch.einsum("oh,bchw,pw->bcop", Ry, x, Rx)


def resample_t(g, size):
    """the transpose of resample(., g's size) applied to g: back to size = (h, w)"""
    Ry, Rx = resample_matrix(size[0], g.shape[-2]), resample_matrix(size[1], g.shape[-1])
    return torch.einsum("oh,bcop,pw->bchw", Ry, g, Rx)


def act_parts(x, mid, out, slope=0.01, scale=None, shift=None):
    """-> (out [B, C, *out], u [B, C, *mid]) in float64"""
    u = resample(affine(x, scale, shift), mid)
    v = torch.where(u > 0, u, slope * u)
    return resample(v, out), u


def act_fwd(x, mid, out, slope=0.01, scale=None, shift=None):
    return act_parts(x, mid, out, slope, scale, shift)[0]


def act_bwd(x, g, mid, slope=0.01, scale=None, shift=None):
    """gradient with respect to y = scale * x + shift; the derivative at u == 0 is slope (torch's convention)"""
    u = resample(affine(x, scale, shift), mid)
    d = torch.where(u > 0, torch.ones_like(u), torch.full_like(u, slope))
    return resample_t(d * resample_t(g.double(), mid), tuple(x.shape[-2:]))


# ---- the rest of a CNO block, float64 ---------------------------------------------------------------------------------
def act(x, in_size, out_size, slope=0.01):
    """CNO_LReLu(in_size, out_size) on x [B, C, H, W] (any H, W), differentiable"""
    return resample(F.leaky_relu(resample(x.double(), (2 * in_size, 2 * in_size)), slope), (out_size, out_size))


def conv(x, w, b=None):
    return F.conv2d(x.double(), w.double(), None if b is None else b.double(), padding=1)


def batchnorm(z, w, b, running_mean, running_var, training, momentum=0.1, eps=1e-5):
    """-> (out, running_mean', running_var') with torch's semantics; the buffers passed in are left alone"""
    rm, rv = running_mean.detach().double().clone(), running_var.detach().double().clone()
    out = F.batch_norm(z.double(), rm, rv, w.double(), b.double(), training, momentum, eps)
    return out, rm, rv
