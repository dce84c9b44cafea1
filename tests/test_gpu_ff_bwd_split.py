"""GPU: the split backward of the fused FeedForward (csrc/ff_bwd_split.hip: k_ffs_adjoint, k_ffs_layer1) against the
path it replaces (k_ff3_bwd_h2 + k_wgrad_h2 with the data gradient, RPDE_FF_BWD_SPLIT=0), through rpde_feedforward_bwd at
the C ABI with dim 64, factor 4, three layers, in the guarded, poisoned buffers of tests/ff_abi.py.

Shapes: P = 8192 (wgrad_h2_ok's minimum: one tile per workgroup on a 256-CU part), 8192 + 3 * 32 + 5 (some workgroups
with a second tile, a partial last tile, idle workgroups in the second round), 4 * 8192 + 17 (several tiles per
workgroup: the LDS stages, panels and running exponents are reused).  Dropout 0.1 and 0.0, LayerNorm on and off.
Weights at the scales of bench.py:time_feedforward; the stash (h1, d1, h2, d2, z3) is what the library's own forward
wrote; one point of grad_out is 1e4 times the rest and sits in the last round of tiles, so that past 8192 points the
running exponents of the du1 panels move after the workgroup's first tile.

Accuracy: every output against a float64 evaluation from the same stash (the LayerNorm / dropout adjoint by autograd,
the chain and the weight gradients as float64 matrix products).  No fixed bound: per output the split path's
relative-L2 error must be at most 2 x the old path's on the same inputs in the same run -- the factor covers another
summation order and nothing more.  dz3, du2 and du1 have the chain's bits by construction and the small gradients are
summed in the chain's order (both paths call the same functions of csrc/ff3_bwd.h), so db1..3, dgamma, dbeta, dW2 and
dW3 -- db0..2, dgamma, dbeta, dW1, dW2 in the names below -- are bit-identical on a part with at most 256 CUs, where both
paths run the same grid: asserted there, reported on a larger part; dx and dW1 differ in the scaling unit of du1 (32
channels instead of 64).
Repeatability: two calls on the split path, identical bits.  Dispatch: recompute mode, grad_x alone and grad_weights
alone do not react to the switch at all (identical bits with RPDE_FF_BWD_SPLIT=0 and without).

Figures of an MI355X run are in DESIGN.md section 4.3."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import ff_abi as A

pytestmark = pytest.mark.gpu

DIM, HID = A.DIM, A.HID
SHAPES = [8192, 8192 + 3 * 32 + 5, 4 * 8192 + 17]
SETTINGS = [(0.1, True), (0.0, True), (0.1, False), (0.0, False)]
EPOCH = 5
SEED = 0x5EED5EED12345
OUTPUTS = ["dx", "dW0", "dW1", "dW2", "db0", "db1", "db2", "dgamma", "dbeta"]
OLD = {"RPDE_FF_BWD_SPLIT": "0"}
SAME_BITS = ["dW1", "dW2", "db0", "db1", "db2", "dgamma", "dbeta"]      # the chain's bits, up to 256 CUs (module docstring)


def _huge_row(P):
    """a point of the last round of tiles: past 256 tiles its workgroup (of a 256-CU part) has seen a tile before it"""
    tiles = (P + 31) // 32
    t = 256 * ((tiles - 1) // 256) + min(7, (tiles - 1) % 256)
    return min(32 * t + 5, P - 1)


@functools.lru_cache(maxsize=2)
def _problem(P, p, layer_norm):
    g = torch.Generator(device="cpu").manual_seed(1000 * P + int(100 * p) + int(layer_norm))
    mk = lambda *shape, s=1.0: torch.randn(*shape, generator=g) * s          # noqa: E731
    w = [mk(HID, DIM, s=0.12), mk(HID, HID, s=0.06), mk(DIM, HID, s=0.06)]
    b = [mk(HID, s=0.1), mk(HID, s=0.1), mk(DIM, s=0.1)]
    gamma, beta = 1.0 + mk(DIM, s=0.1), mk(DIM, s=0.1)
    x, res, gout = mk(P, DIM), mk(P, DIM), mk(P, DIM)
    gout[_huge_row(P)] *= 1e4
    return dict(P=P, p=p, layer_norm=layer_norm, w=w, b=b, gamma=gamma, beta=beta, x=x, res=res, gout=gout)


class _Call:
    """one forward of `prob` in guarded buffers (stash or recompute mode), then any number of backward calls on it"""

    def __init__(self, dev, prob, recompute=False):
        from rpde import _lib, ops
        self.lib, self._lib, self.dev, self.prob = _lib.load(), _lib, dev, prob
        P, ln = prob["P"], prob["layer_norm"]
        self.w = [t.to(dev).contiguous() for t in prob["w"]]
        self.b = [t.to(dev).contiguous() for t in prob["b"]]
        self.gamma = prob["gamma"].to(dev) if ln else None
        self.beta = prob["beta"].to(dev) if ln else None
        self.bufs = A.Buffers(dev)
        self.X = self.bufs.new("x", (P, DIM), prob["x"])
        self.R = self.bufs.new("residual", (P, DIM), prob["res"])
        self.out = self.bufs.new("out", (P, DIM))
        self.z3 = self.bufs.new("z_last", (P, DIM))
        self.hs = [self.bufs.new(f"hs{l}", (P, HID)) for l in range(2)]
        self.ds = None if recompute else [self.bufs.new(f"ds{l}", (P, HID)) for l in range(2)]
        self.G = self.bufs.new("grad_out", (P, DIM), prob["gout"])
        self.wa, self.ba = _lib.ptr_array(self.w), _lib.ptr_array(self.b)
        self.ep = ops.drop_epoch(dev) if prob["p"] > 0.0 else None
        self.fp = _lib.FFParams(3, DIM, 4, int(ln), 1e-5, prob["p"], SEED, _lib.ACT["identity"],
                                C.cast(self.wa, C.POINTER(C.c_void_p)), C.cast(self.ba, C.POINTER(C.c_void_p)),
                                _lib.ptr(self.gamma), _lib.ptr(self.beta), self.ep.data_ptr() if self.ep is not None else None)
        self.st = _lib.stream_ptr()
        assert int(self.lib.rpde_feedforward_is_fused(DIM, 4, 3, P)) == 1
        nws = int(self.lib.rpde_feedforward_fwd_ws_bytes(DIM, 4, 3))
        ws = self.bufs.new_bytes("fwd_ws", nws)
        self._epoch(EPOCH)
        try:
            _lib.check(self.lib.rpde_feedforward_fwd(C.byref(self.fp), self.X.ptr, self.R.ptr, A.ptr_list(self.hs),
                                                     A.ptr_list(self.ds), self.z3.ptr, self.out.ptr, P, ws.ptr, nws, self.st),
                       "feedforward_fwd")
            torch.cuda.synchronize()
        finally:
            self._epoch(0)
        self.bufs.check(["out", "z_last", "hs0", "hs1"] + ([] if recompute else ["ds0", "ds1"]), f"forward P={P}")

    def _epoch(self, v):
        if self.ep is not None:
            self.ep.fill_(v)

    def stash(self):
        return {k: self.bufs.all[k].t.cpu().clone() for k in ("hs0", "hs1", "ds0", "ds1", "z_last")}

    def backward(self, env=None, grad_x=True, grad_weights=True):
        P, ln, lib = self.prob["P"], self.prob["layer_norm"], self.lib
        bufs = self.bufs
        gx = bufs.new("dx", (P, DIM)) if grad_x else None
        gW = [bufs.new(f"dW{l}", tuple(self.w[l].shape)) for l in range(3)] if grad_weights else None
        gb = [bufs.new(f"db{l}", tuple(self.b[l].shape)) for l in range(3)]
        gga = bufs.new("dgamma", (DIM,)) if ln else None
        gbe = bufs.new("dbeta", (DIM,)) if ln else None
        names = [k for k in OUTPUTS if (k != "dx" or grad_x) and (not k.startswith("dW") or grad_weights)
                 and (ln or k not in ("dgamma", "dbeta"))]
        self._epoch(EPOCH)
        try:
            with A.Env(env):                                # (the workspace query reads the switches too)
                nws = int(lib.rpde_feedforward_ws_bytes(P, DIM, 4, 3))
                ws = bufs.new_bytes("bwd_ws", nws)
                self._lib.check(lib.rpde_feedforward_bwd(C.byref(self.fp), self.X.ptr, A.ptr_list(self.hs), A.ptr_list(self.ds),
                                                         self.z3.ptr, self.G.ptr, A.ptr_or_none(gx), A.ptr_list(gW),
                                                         A.ptr_list(gb), A.ptr_or_none(gga), A.ptr_or_none(gbe), P, ws.ptr, nws,
                                                         self.st), "feedforward_bwd")
                torch.cuda.synchronize()
        finally:
            self._epoch(0)
        bufs.check(names, f"backward P={P} env={env}")
        res = {k: bufs.all[k].t.cpu().clone() for k in names}
        for k in names + ["bwd_ws"]:
            del bufs.all[k]
        return res


def _reference(prob, stash):
    """float64, from what the forward saved: h1, d1, h2, d2 (d = gelu'(u) * dropout factor) and z3"""
    from oracle import dropout_mask as D
    P, p, ln = prob["P"], prob["p"], prob["layer_norm"]
    W = [t.double() for t in prob["w"]]
    h1, h2, d1, d2 = (stash[k].double() for k in ("hs0", "hs1", "ds0", "ds1"))
    z3 = stash["z_last"].double().requires_grad_()
    gamma, beta = prob["gamma"].double().requires_grad_(), prob["beta"].double().requires_grad_()
    t = z3 * D.layer_mask(SEED, 2, EPOCH, p, P, DIM).reshape(P, DIM) if p > 0.0 else z3
    y = F.layer_norm(t, (DIM,), gamma, beta, 1e-5) if ln else t
    (y * prob["gout"].double()).sum().backward()
    dz3 = z3.grad
    du2 = (dz3 @ W[2]) * d2
    du1 = (du2 @ W[1]) * d1
    ref = {"dx": du1 @ W[0], "dW0": du1.t() @ prob["x"].double(), "dW1": du2.t() @ h1, "dW2": dz3.t() @ h2,
           "db0": du1.sum(0), "db1": du2.sum(0), "db2": dz3.sum(0)}
    if ln:
        ref["dgamma"], ref["dbeta"] = gamma.grad, beta.grad
    return ref


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("p,layer_norm", SETTINGS, ids=[f"drop{p}-{'ln' if ln else 'noln'}" for p, ln in SETTINGS])
@pytest.mark.parametrize("P", SHAPES)
def test_split_backward_against_the_chain(gpu_device, P, p, layer_norm):
    prob = _problem(P, p, layer_norm)
    call = _Call(gpu_device, prob)
    ref = _reference(prob, call.stash())
    new = call.backward()
    again = call.backward()
    old = call.backward(env=OLD)
    names = [k for k in OUTPUTS if k in ref]
    assert set(new) == set(old) == set(names)
    e_new = {k: A.rel(new[k], ref[k]) for k in names}
    e_old = {k: A.rel(old[k], ref[k]) for k in names}
    same = [k for k in names if _bits_equal(new[k], old[k])]
    print(f"\n[ff-bwd-split] P={P} p={p} ln={int(layer_norm)} same_bits_as_old={','.join(same)}")
    for k in names:
        print(f"[ff-bwd-split]   {k:7s} split {e_new[k]:.3e}  old {e_old[k]:.3e}  ratio {e_new[k] / max(e_old[k], 1e-300):.2f}")
    # the switch reaches the kernels: the first layer's gradients come from another kernel (dW0 alone can coincide where
    # the two halves of every du1 panel share their exponent)
    assert not (_bits_equal(new["dx"], old["dx"]) and _bits_equal(new["dW0"], old["dW0"])), "RPDE_FF_BWD_SPLIT=0 changed nothing"
    for k in names:
        assert e_new[k] <= 2.0 * e_old[k], (k, e_new[k], e_old[k])
    for k in names:
        assert _bits_equal(new[k], again[k]), (k, "not reproducible")
    if torch.cuda.get_device_properties(gpu_device).multi_processor_count <= 256:
        for k in SAME_BITS:
            assert k not in names or k in same, (k, "not the chain's bits")


def test_split_dispatch_leaves_the_other_calls_alone(gpu_device):
    """recompute mode, grad_x alone, grad_weights alone: the old kernels, whatever the switch says"""
    prob = _problem(SHAPES[1], 0.1, True)
    stash = _Call(gpu_device, prob)
    for what, kw in (("grad_x only", dict(grad_weights=False)), ("grad_weights only", dict(grad_x=False))):
        a, b = stash.backward(**kw), stash.backward(env=OLD, **kw)
        for k in a:
            assert _bits_equal(a[k], b[k]), (what, k)
    rec = _Call(gpu_device, prob, recompute=True)
    a, b = rec.backward(), rec.backward(env=OLD)
    for k in a:
        assert _bits_equal(a[k], b[k]), ("recompute", k)
