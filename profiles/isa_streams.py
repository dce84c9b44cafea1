"""Instruction streams of the compiled gfx950 kernels, for refactors that must not move a hot kernel.

    python profiles/isa_streams.py dump OUT.json [--csrc DIR] [--streams DIR] [fused_spectral fused_mix lifted_spectral ...]
    python profiles/isa_streams.py compare PARENT.json CHANGE.json

`dump` compiles each source of DIR (default: resolution-pde_amd/csrc) to device assembly with the flags of rpde/build.py
and records per kernel: a hash and the length of its instruction stream (comments dropped except the `cw_mark` /
`cw_wait` lines of csrc/cw.h, debug directives dropped, basic-block labels renumbered per kernel so that a kernel added
or removed elsewhere in the file changes nothing), .vgpr_count, .sgpr_count, LDS and scratch bytes.  `compare` prints
the table same / changed and exits 1 if a kernel gained scratch or changed its LDS.  No GPU needed.  To compare against
another commit, check its csrc out somewhere (git worktree) and point --csrc at it.
"""
from __future__ import annotations

import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "resolution-pde_amd"))
from rpde import build as rb  # noqa: E402

DEFAULT = ["fused_spectral", "fused_mix", "lifted_spectral"]
DROP = (".loc", ".file", ".cfi", ".p2align", ";")


def _short(name):
    """_ZN4rpde19k_dft_synthesis3_h2ILi0ELi1EEEvNS_4SynPE -> k_dft_synthesis3_h2<0,1>; bool arguments (Lb0E / Lb1E)
    are kept as false / true, so that every instance of k_wgrad_h2<.., ACT, DG> or k_ff3_bwd_h2<RECOMP> has its own row"""
    m = re.match(r"_ZN4rpde(\d+)", name)
    if not m:
        return name
    base, rest = name[m.end():m.end() + int(m.group(1))], name[m.end() + int(m.group(1)):]
    t = re.match(r"I((?:L[ib]\d+E)+)E", rest)
    if not t:
        return base
    args = [("false", "true")[int(v)] if k == "b" else v for k, v in re.findall(r"L([ib])(\d+)E", t.group(1))]
    return base + "<" + ",".join(args) + ">"


def stream(body):
    """instruction lines of one kernel, normalised"""
    out, labels = [], {}
    for raw in body:
        t = raw.strip()
        if not t or t.startswith(DROP):
            if "cw_" not in t:
                continue
        if ";" in t and "cw_" not in t:
            t = t.split(";", 1)[0].rstrip()
        t = re.sub(r"\s+", " ", t)
        if t:
            out.append(t)
    for t in out:                                       # labels in order of definition
        m = re.match(r"(\.LBB\d+_\d+):", t)
        if m:
            labels[m.group(1)] = ".L%d" % len(labels)
    return [re.sub(r"\.LBB\d+_\d+", lambda m: labels.get(m.group(0), m.group(0)), t) for t in out]


def kernels_of(csrc, source, keep=None):
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, source + ".s")
        flags = [f for f in rb.FLAGS if not f.startswith("-I")] + ["-I" + rb.INCLUDE, "-I" + csrc]
        cmd = [rb._hipcc(), *flags, "--cuda-device-only", "-S", os.path.join(csrc, source + ".hip"), "-o", asm]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit(r.stderr[-4000:])
        text = open(asm).read().split("\n")
    meta, cur = {}, None                                # the metadata note at the end: one record per kernel
    for line in text:
        m = re.match(r"\s+(?:- )?\.(\w+):\s+(\S+)\s*$", line)
        if not m:
            continue
        if line.lstrip().startswith("- ."):
            cur = {}
        if cur is None:
            continue
        key, val = m.group(1), m.group(2)
        if key in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size"):
            cur[key] = int(val)
        elif key == "name":
            meta[val] = cur
    res = {}
    for i, line in enumerate(text):
        m = re.match(r"(_Z\w+):", line)
        if m and m.group(1) in meta:
            end = next(j for j in range(i, len(text)) if ".Lfunc_end" in text[j])
            s = stream(text[i + 1:end])
            k = meta[m.group(1)]
            if keep:
                open(os.path.join(keep, m.group(1) + ".s"), "w").write("\n".join(s) + "\n")
            res[m.group(1)] = {"hash": hashlib.sha256("\n".join(s).encode()).hexdigest()[:16], "insts": len(s),
                               "vgpr": k["vgpr_count"], "sgpr": k["sgpr_count"], "lds": k["group_segment_fixed_size"],
                               "scratch": k["private_segment_fixed_size"]}
    return res


def dump(out, csrc, sources, keep=None):
    res = {}
    for s in sources:
        ks = kernels_of(csrc, s, keep)
        res[s] = {_short(k): v for k, v in ks.items()}
        print(f"{s}: {len(ks)} kernels", flush=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)


def compare(pa, pb):
    a, b = json.load(open(pa)), json.load(open(pb))
    bad = 0
    for src in sorted(set(a) | set(b)):
        print(f"== {src}.hip")
        print(f"{'kernel':36s} {'stream':8s} {'insts':>13s} {'vgpr':>9s} {'sgpr':>9s} {'lds':>15s} {'scratch':>7s}")
        ka, kb = a.get(src, {}), b.get(src, {})
        for name in sorted(set(ka) | set(kb)):
            x, y = ka.get(name), kb.get(name)
            if x is None or y is None:
                z = x or y
                print(f"{name:36s} {'new' if x is None else 'gone':8s} {z['insts']:>13d} {z['vgpr']:>9d} {z['sgpr']:>9d} {z['lds']:>15d} "
                      f"{z['scratch']:>7d}")
                bad += y is not None and y["scratch"] > 0
                continue
            same = x["hash"] == y["hash"]
            pair = lambda k: str(x[k]) if x[k] == y[k] else f"{x[k]}->{y[k]}"
            print(f"{name:36s} {'same' if same else 'CHANGED':8s} {pair('insts'):>13s} {pair('vgpr'):>9s} {pair('sgpr'):>9s} "
                  f"{pair('lds'):>15s} {pair('scratch'):>7s}")
            if y["scratch"] > x["scratch"] or y["lds"] != x["lds"]:
                bad += 1
    if bad:
        print(f"{bad} kernel(s) gained scratch or changed LDS")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) >= 3 and sys.argv[1] == "dump":
        args = sys.argv[3:]
        csrc = rb.CSRC
        if "--csrc" in args:
            i = args.index("--csrc")
            csrc = os.path.abspath(args[i + 1])
            del args[i:i + 2]
        keep = None
        if "--streams" in args:                          # also write each normalised stream to DIR/<mangled name>.s
            i = args.index("--streams")
            keep = args[i + 1]
            os.makedirs(keep, exist_ok=True)
            del args[i:i + 2]
        dump(sys.argv[2], csrc, args or DEFAULT, keep)
        sys.exit(0)
    sys.exit(__doc__)
