"""float64 restatement of the CNO activation (reference models/CNO1d.py:30-45), test infrastructure only.  Its
resampling matrices come from F.interpolate applied to an identity, never from the tables of the code under test."""
import functools

import torch
import torch.nn.functional as F


@functools.lru_cache(maxsize=None)
def resample_matrix(n_in: int, n_out: int) -> torch.Tensor:
    """[n_out, n_in] float64: F.interpolate(mode="bicubic", antialias=True) on a (1, n_in) image, column by column"""
    eye = torch.eye(n_in, dtype=torch.float64).reshape(n_in, 1, 1, n_in)
    cols = F.interpolate(eye, size=(1, n_out), mode="bicubic", antialias=True)
    return cols.reshape(n_in, n_out).t().contiguous()


def affine(x, scale, shift):
    x = x.double()
    return x if scale is None else x * scale.double().view(1, -1, 1) + shift.double().view(1, -1, 1)


def act_parts(x, n_mid, n_out, slope=0.01, scale=None, shift=None):
    """-> (out [B, C, n_out], u [B, C, n_mid]) in float64"""
    U, D = resample_matrix(x.shape[-1], n_mid), resample_matrix(n_mid, n_out)
    u = affine(x, scale, shift) @ U.t()
    v = torch.where(u > 0, u, slope * u)
    return v @ D.t(), u


def act_fwd(x, n_mid, n_out, slope=0.01, scale=None, shift=None):
    return act_parts(x, n_mid, n_out, slope, scale, shift)[0]


def act_bwd(x, g, n_mid, n_out, slope=0.01, scale=None, shift=None):
    """gradient with respect to y = scale * x + shift; the derivative at u == 0 is slope (torch's convention)"""
    U, D = resample_matrix(x.shape[-1], n_mid), resample_matrix(n_mid, n_out)
    u = affine(x, scale, shift) @ U.t()
    d = torch.where(u > 0, torch.ones_like(u), torch.full_like(u, slope))
    return (d * (g.double() @ D)) @ U


def min_margin(u):
    """smallest |u| over its rms: how close the nearest mid pre-activation is to the LeakyReLU kink"""
    return float(u.abs().min() / u.pow(2).mean().sqrt())


# ---- the rest of a CNO block and the whole model, float64 -----------------------------------------------------------
def act(x, in_size, out_size, slope=0.01):
    """CNO_LReLu(in_size, out_size) on x [B, C, n] (any n), differentiable"""
    U, D = resample_matrix(x.shape[-1], 2 * in_size), resample_matrix(2 * in_size, out_size)
    return F.leaky_relu(x.double() @ U.t(), slope) @ D.t()


def conv(x, w, b=None):
    return F.conv1d(x.double(), w.double(), None if b is None else b.double(), padding=1)


def batchnorm(z, w, b, running_mean, running_var, training, momentum=0.1, eps=1e-5):
    """-> (out, running_mean', running_var') with torch's semantics; the buffers passed in are left alone"""
    rm, rv = running_mean.detach().double().clone(), running_var.detach().double().clone()
    out = F.batch_norm(z.double(), rm, rv, w.double(), b.double(), training, momentum, eps)
    return out, rm, rv


def cno1d_forward(sd, x, size, N_layers, N_res, N_res_neck, use_bn, training):
    """CNO1d.forward from a state_dict `sd` of float64 tensors (parameters may require grad) -> (y, {buffer: new value})"""
    L, new = N_layers, {}
    enc_sizes = [size // 2 ** i for i in range(L + 1)]
    dec_sizes = [size // 2 ** (L - i) for i in range(L + 1)]

    def bn(prefix, z):
        if not use_bn:
            return z
        out, rm, rv = batchnorm(z, sd[prefix + ".weight"], sd[prefix + ".bias"], sd[prefix + ".running_mean"],
                                sd[prefix + ".running_var"], training)
        if training:
            new[prefix + ".running_mean"], new[prefix + ".running_var"] = rm, rv
            new[prefix + ".num_batches_tracked"] = sd[prefix + ".num_batches_tracked"] + 1
        return out

    def block(prefix, z, in_size, out_size, with_bn=True):
        z = conv(z, sd[prefix + ".convolution.weight"], sd[prefix + ".convolution.bias"])
        return act(bn(prefix + ".batch_norm", z) if with_bn else z, in_size, out_size)

    def lift_project(prefix, z):
        z = block(prefix + ".inter_CNOBlock", z, size, size, with_bn=False)
        return conv(z, sd[prefix + ".convolution.weight"], sd[prefix + ".convolution.bias"])

    def resnet(prefix, z, n, blocks):
        for k in range(blocks):
            p = f"{prefix}.res_nets.{k}"
            h = conv(z, sd[p + ".convolution1.weight"], sd[p + ".convolution1.bias"])
            h = act(bn(p + ".batch_norm1", h), n, n)
            h = conv(h, sd[p + ".convolution2.weight"], sd[p + ".convolution2.bias"])
            z = z + bn(p + ".batch_norm2", h)
        return z

    x = lift_project("lift", x.double())
    skip = []
    for i in range(L):
        skip.append(resnet(f"res_nets.{i}", x, enc_sizes[i], N_res))
        x = block(f"encoder.{i}", x, enc_sizes[i], enc_sizes[i + 1])
    x = resnet("res_net_neck", x, enc_sizes[L], N_res_neck)
    for i in range(L):
        if i == 0:
            x = block(f"ED_expansion.{L}", x, enc_sizes[L], dec_sizes[0])
        else:
            x = torch.cat((x, block(f"ED_expansion.{L - i}", skip[-i], enc_sizes[L - i], dec_sizes[i])), 1)
        x = block(f"decoder.{i}", x, dec_sizes[i], dec_sizes[i + 1])
    x = torch.cat((x, block("ED_expansion.0", skip[0], enc_sizes[0], dec_sizes[L])), 1)
    return lift_project("project", x), new
