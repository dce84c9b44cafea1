"""The dropout-mask restatement (oracle/dropout_mask.py) against the one definition the kernels use
(resolution-pde_amd/csrc/drop_hash.h), bit for bit, and the statistical properties of the masks it restates.

No GPU: the header also builds with a plain C++ compiler, so a tiny host program evaluates exactly the functions the
kernels inline.  The GPU parity tests (tests/test_gpu_dropout_parity.py) then only need to trust this restatement."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from oracle import dropout_mask as D

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "resolution-pde_amd", "csrc")

HOST_PROGRAM = r"""
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include "drop_hash.h"
// stdin: "seed layer epoch p_bits id" per line (unsigned decimal; p as float32 bits)
// stdout: "layer_seed thresh scale_bits s1_bits [s4_0 s4_1 s4_2 s4_3 when id % 4 == 0]" in hex
int main() {
  unsigned long long seed, epoch, id;
  unsigned pbits;
  int layer;
  while (std::scanf("%llu %d %llu %u %llu", &seed, &layer, &epoch, &pbits, &id) == 5) {
    float p;
    std::memcpy(&p, &pbits, 4);
    const uint64_t ep = epoch;
    const uint64_t ls = rpde::layer_seed(seed, layer);
    const rpde::DropCfg d = rpde::drop_resolve(rpde::make_drop(p, ls, &ep));
    uint32_t sb, s1;
    std::memcpy(&sb, &d.scale, 4);
    const float v = rpde::drop_scale1(d, id);
    std::memcpy(&s1, &v, 4);
    std::printf("%" PRIx64 " %x %x %x", ls, d.thresh, sb, s1);
    if (id % 4 == 0) {
      float s[4];
      rpde::drop_scale4(d, id, s);
      for (int j = 0; j < 4; ++j) { uint32_t b; std::memcpy(&b, &s[j], 4); std::printf(" %x", b); }
    }
    std::printf("\n");
  }
  return 0;
}
"""


def _cxx():
    for cand in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if cand and shutil.which(cand):
            return shutil.which(cand)
    return None


def _f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def _queries():
    rng = np.random.default_rng(20261016)
    seeds = [0, 1, 0x0123456789ABCDEF, (1 << 64) - 1, int(rng.integers(0, 2 ** 62)), 1 << 32]
    epochs = [0, 1, (1 << 40) + 3]
    ps = [2.0 ** -17, 0.1, 0.2, 0.5, 0.9999]
    two32 = 1 << 32
    ids = list(range(0, 37))                                          # every lane of the first groups, odd ids too
    ids += [two32 - 9 + k for k in range(18)]                         # around 2^32 (high word of the id)
    ids += [4 * two32 - 5 + k for k in range(10)]                     # around 2^34 (high word of the group)
    ids += [(1 << 40) + 7, (1 << 52) + 2, (1 << 63) + 1, (1 << 64) - 1, (1 << 64) - 4]
    ids += [int(v) for v in rng.integers(0, 2 ** 63, 40, dtype=np.int64)]
    out = []
    for s in seeds:
        for e in epochs:
            for p in ps:
                layer = int(rng.integers(0, 9))
                for i in ids:
                    out.append((s, layer, e, p, i))
    return out


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = _cxx()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("drop_hash")
    src, exe = d / "drop_hash_host.cpp", d / "drop_hash_host"
    src.write_text(HOST_PROGRAM)
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-I" + CSRC, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def test_restatement_matches_the_header_bit_for_bit(host_program):
    qs = _queries()
    assert len(qs) > 5000
    stdin = "".join(f"{s} {l} {e} {_f32_bits(p)} {i}\n" for s, l, e, p, i in qs)
    r = subprocess.run([host_program], input=stdin, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(qs)
    bad = []
    for (s, l, e, p, i), line in zip(qs, lines):
        f = [int(t, 16) for t in line.split()]
        ls = D.layer_seed(s, l)
        want = [ls, D.threshold(p), _f32_bits(D.scale(p)),
                _f32_bits(float(D.factor(ls, e, p, np.array([i], dtype=np.uint64))[0]))]
        if i % 4 == 0:
            want += [_f32_bits(float(v)) for v in D.factor(ls, e, p, np.arange(i, i + 4, dtype=np.uint64))]
        if f != want:
            bad.append(((s, l, e, p, i), f, want))
    assert not bad, f"{len(bad)} mismatches, first: {bad[:3]}"
    # the queries reach both outcomes and every lane of a group
    fac = np.array([int(line.split()[3], 16) for line in lines])
    assert (fac == 0).any() and (fac != 0).any()


def test_threshold_and_scale_formulas():
    assert D.threshold(0.0) == 0 and D.scale(0.0) == 1.0
    assert D.threshold(0.1) == 6554 and D.threshold(0.2) == 13107 and D.threshold(0.5) == 32768
    # the keep factor follows the quantised threshold, not 1 / (1 - p): at p = 0.1 they differ by ~6.8e-6
    assert abs(D.scale(0.1) - 1 / (1 - 6554 / 65536)) < 1e-7
    assert abs(D.scale(0.1) / (1 / 0.9) - 1) > 5e-6
    # documented clamps: any p > 0 drops something (thresh >= 1), p -> 1 keeps something (thresh <= 65535)
    assert D.threshold(1e-12) == 1 and D.threshold(2.0 ** -18) == 1 and D.threshold(2.0 ** -17) == 1
    assert D.threshold(1 - 2.0 ** -18) == 65535 and D.threshold(1 - 2.0 ** -17) == 65535
    # inside [2^-16, 1 - 2^-16] the effective rate is within half a quantum of p
    for p in np.linspace(2.0 ** -16, 1 - 2.0 ** -16, 20001, dtype=np.float32):
        assert abs(D.threshold(float(p)) / 65536 - float(p)) <= 2.0 ** -17


# ---- statistics of the restated masks: every bound in standard deviations of the binomial under independence ----
N_POINTS, WIDTH = 4096, 256          # 2^20 elements, FFNO2D's hidden width
Z = 5.0


def _keep(seed, layer, epoch, p, offset=0, points=N_POINTS, width=WIDTH):
    return D.layer_mask(seed, layer, epoch, p, points, width, offset).numpy() != 0


def _rate_ok(k, p_keep):
    n = k.size
    sd = np.sqrt(p_keep * (1 - p_keep) / n)
    return abs(k.mean() - p_keep) <= Z * sd, (k.mean(), p_keep, sd)


@pytest.mark.parametrize("p", [0.1, 0.2, 0.5])
@pytest.mark.parametrize("offset", [0, (1 << 32) - 2 ** 19])
def test_keep_rate_overall_and_per_residue(p, offset):
    """keep rate = 1 - thresh/65536 overall and on every residue class mod 4 / 64 / 256 of the id (the lane of a
    group, the wave lane, the hidden feature), also across the 2^32 boundary of the id"""
    keep = _keep(0xC0FFEE, 1, 0, p, offset).reshape(-1)
    pk = 1 - D.threshold(p) / 65536
    ok, info = _rate_ok(keep, pk)
    assert ok, info
    ids = np.arange(keep.size, dtype=np.uint64) + np.uint64(offset)
    for mod in (4, 64, 256):
        classes = (ids % np.uint64(mod)).astype(np.int64)
        cnt = np.bincount(classes, minlength=mod)
        kept = np.bincount(classes, weights=keep, minlength=mod)
        sd = np.sqrt(pk * (1 - pk) / cnt)
        # the maximum of `mod` classes: allow for the extreme of that many draws (Bonferroni)
        z = Z + np.sqrt(2 * np.log(mod))
        worst = np.abs(kept / cnt - pk) / sd
        assert worst.max() <= z, (mod, worst.max(), int(worst.argmax()))


def _corr_ok(a, b, p_keep):
    """fraction both kept vs p_keep^2: independent masks agree there within Z standard deviations"""
    n = a.size
    both = (a & b).mean()
    q = p_keep * p_keep
    sd = np.sqrt(q * (1 - q) / n)
    return abs(both - q) <= Z * sd, (both, q, sd)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_masks_are_uncorrelated(p):
    """no correlation between layers of one seed, epochs e and e+1, adjacent points, or seeds one bit apart"""
    pk = 1 - D.threshold(p) / 65536
    seed = 0x5DEECE66D
    base = _keep(seed, 0, 7, p)
    pairs = {
        "layer 0 vs 1": (base, _keep(seed, 1, 7, p)),
        "layer 1 vs 2": (_keep(seed, 1, 7, p), _keep(seed, 2, 7, p)),
        "epoch 7 vs 8": (base, _keep(seed, 0, 8, p)),
        "epoch 0 vs 1": (_keep(seed, 0, 0, p), _keep(seed, 0, 1, p)),
        "adjacent points": (base[:-1], base[1:]),
        "adjacent features": (base[:, :-1], base[:, 1:]),
    }
    for bit in (0, 1, 31, 32, 63):
        # a raw seed one bit apart (the layer seed mixes it; the epoch fold does not)
        pairs[f"seed bit {bit}"] = (base, _keep(seed ^ (1 << bit), 0, 7, p))
    for name, (a, b) in pairs.items():
        ok, info = _corr_ok(a.reshape(-1), b.reshape(-1), pk)
        assert ok, (name, info)


def test_hash_level_seed_bits_change_the_mask():
    """the raw hash (no layer-seed mixing): a one-bit change of the resolved seed, low or high word, gives an
    unrelated mask -- this is what the epoch fold relies on"""
    p, pk = 0.5, 1 - D.threshold(0.5) / 65536
    ids = np.arange(1 << 20, dtype=np.uint64)
    a = D.keep(0x123456789, 0, p, ids)
    for bit in (0, 5, 31, 32, 40, 63):
        b = D.keep(0x123456789 ^ (1 << bit), 0, p, ids)
        ok, info = _corr_ok(a, b, pk)
        assert ok, (bit, info)


def test_layer_mask_layout():
    """ids are point * out_features + feature (+ offset); feedforward_masks gives hidden widths then dim"""
    m = D.layer_mask(9, 2, 3, 0.3, 5, 12, id_offset=40).numpy()
    flat = D.factor(D.layer_seed(9, 2), 3, 0.3, np.arange(40, 40 + 60, dtype=np.uint64))
    assert np.array_equal(m.reshape(-1), flat)
    ms = D.feedforward_masks(9, 3, 0.3, 5, 8, 3, 4)
    assert [tuple(t.shape) for t in ms] == [(5, 24), (5, 24), (5, 24), (5, 8)]
    assert set(np.unique(ms[0].numpy())) <= {0.0, D.scale(0.3)}
    assert np.all(D.layer_mask(9, 2, 3, 0.0, 5, 12).numpy() == 1.0)
