"""float64 restatement of the per-frequency error decomposition (test infrastructure only; the product tree does not
import it), the fixture cases and their inputs.

    1-D  amp[k] = sqrt(w_k / H * sum_{b,c} |Z[b,c,k]|^2),  Z = rfft(z),  w_k = 1 at DC and (even H) Nyquist, else 2
    2-D  amp[i] = sqrt(1/(H W) * sum_{(ky,kx) in bin i} w_kx sum_{b,c} |Z[b,c,ky,kx]|^2),  Z = rfft2(z)
         bins: edges np.linspace(0, 0.5, nb + 1), r = sqrt(fftfreq(H)^2 + rfftfreq(W)^2) as a float32 torch tensor,
         edges[i] <= r < edges[i+1]; r >= 0.5 belongs to no bin; centres (edges[i] + edges[i+1]) / 2

with z = y_hat - y for the error and z = y for the solution, everything in float64.  The keyword arguments switch on
deliberately WRONG variants: the tests use them to show that the comparison can see a wrong answer."""
from __future__ import annotations

import numpy as np
import torch

# (name, shape, num_modes (1-D) / num_radial_bins (2-D), s, seed)
CASES_1D = [
    ("freq_1d_64", (5, 1, 64), None, 1e-2, 3),
    ("freq_1d_64_m16", (5, 1, 64), 16, 1e-2, 3),
    ("freq_1d_512", (3, 2, 512), None, 1e-2, 3),
    ("freq_1d_512_m16", (3, 2, 512), 16, 1e-2, 3),
    ("freq_1d_1024", (7, 1, 1024), None, 1e-2, 3),
    ("freq_1d_1024_m16", (7, 1, 1024), 16, 1e-2, 3),
    ("freq_1d_1023", (3, 1, 1023), None, 1e-2, 3),
    ("freq_1d_1023_m16", (3, 1, 1023), 16, 1e-2, 3),
    ("freq_1d_96", (5, 3, 96), None, 1e-2, 3),
    ("freq_1d_96_m16", (5, 3, 96), 16, 1e-2, 3),
    ("freq_1d_1024_good", (6, 1, 1024), None, 1e-4, 3),
]
CASES_2D = [
    ("freq_2d_64", (5, 1, 64, 64), 64, 1e-2, 3),
    ("freq_2d_256", (3, 1, 256, 256), 64, 1e-2, 3),
    ("freq_2d_96x160", (3, 2, 96, 160), 32, 1e-2, 3),
    ("freq_2d_63x65", (5, 1, 63, 65), 16, 1e-2, 3),
    ("freq_2d_32_b64", (7, 1, 32, 32), 64, 1e-2, 3),
    ("freq_2d_64_c3", (3, 3, 64, 64), 64, 1e-2, 3),
    ("freq_2d_128_good", (3, 1, 128, 128), 64, 1e-4, 3),
]
CASES = {c[0]: c for c in CASES_1D + CASES_2D}


def make_inputs(shape, s, seed):
    """(prediction, target), float32: a smooth field plus a per-channel mean (so that the DC weight matters), and white
    noise of size s with a mean on top of it for the prediction (so that Nyquist and the corners carry error)"""
    from tests.golden import synth
    y = synth.smooth_field(shape, seed, "y")
    mean = 0.5 * (torch.arange(shape[1], dtype=torch.float32) + 1.0)
    y = y + mean.view(1, -1, *([1] * (len(shape) - 2)))
    e = synth.rand_tensor(shape, seed, "e") + 0.5
    return (y + s * e).float(), y.float()


def _w(n, nk, edge=1.0, interior=2.0):
    w = np.full(nk, interior)
    w[0] = edge
    if n % 2 == 0 and nk == n // 2 + 1:
        w[n // 2] = edge
    return w


def ref_1d(y_hat, y, num_modes=None, edge_weight=1.0, interior_weight=2.0):
    """-> (error, solution, frequencies); edge_weight=2 / interior_weight=1 are wrong on purpose"""
    y_hat, y = y_hat.double(), y.double()
    H = y.shape[-1]
    nk = H // 2 + 1
    num_modes = min(num_modes or nk, nk)
    w = _w(H, nk, edge_weight, interior_weight)
    out = []
    for z in (y_hat - y, y):
        e = (torch.fft.rfft(z, dim=-1).abs() ** 2).sum(dim=(0, 1)).numpy()
        out.append(np.sqrt(w * e / H)[:num_modes])
    return out[0], out[1], torch.fft.rfftfreq(H).numpy()[:num_modes]      # float32, as the reference returns them


def bin_table(H, W, nb, closed_right=False, corners_in_last=False):
    """int64 [H, W//2+1]: bin of every half-spectrum entry, -1 for none"""
    r = torch.sqrt(torch.fft.fftfreq(H).view(-1, 1) ** 2 + torch.fft.rfftfreq(W).view(1, -1) ** 2)
    assert r.dtype == torch.float32
    edges = np.linspace(0, 0.5, nb + 1)
    bins = torch.full(r.shape, -1, dtype=torch.int64)
    for i in range(nb):
        m = ((r > edges[i]) & (r <= edges[i + 1])) if closed_right else ((r >= edges[i]) & (r < edges[i + 1]))
        bins[m] = i
    if corners_in_last:
        bins[r >= 0.5] = nb - 1
    return bins.numpy(), (edges[:-1] + edges[1:]) / 2


def ref_2d(y_hat, y, num_radial_bins=64, edge_weight=1.0, closed_right=False, corners_in_last=False):
    y_hat, y = y_hat.double(), y.double()
    H, W = y.shape[-2:]
    bins, centres = bin_table(H, W, num_radial_bins, closed_right, corners_in_last)
    w = _w(W, W // 2 + 1, edge_weight)[None, :]
    out = []
    for z in (y_hat - y, y):
        e = (torch.fft.rfft2(z, dim=(-2, -1)).abs() ** 2).sum(dim=(0, 1)).numpy() * w
        amp = np.zeros(num_radial_bins)
        ok = bins >= 0
        np.add.at(amp, bins[ok], e[ok])
        out.append(np.sqrt(amp / (H * W)))
    return out[0], out[1], centres


def wrong_variants(dims):
    """{label: kwargs of ref_1d / ref_2d that give a wrong answer}"""
    if dims == 1:
        return {"a: weight 2 on DC and Nyquist": dict(edge_weight=2.0), "d: interior weight 1": dict(interior_weight=1.0)}
    return {"a: weight 2 on DC and Nyquist": dict(edge_weight=2.0), "b: bins closed on the right": dict(closed_right=True),
            "c: corners in the last bin": dict(corners_in_last=True)}


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def load(name):
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}
