#!/usr/bin/env python3
"""Compare the device code of two csrc directories kernel by kernel: the check a refactor that must not
move the machine code is held to.  Each .hip file is compiled on both sides to device-only gfx950
assembly with the Makefile's CXXFLAGS (about 35 s per file, at most 16 jobs), the output is split per
kernel symbol, and a kernel is identical when its instruction text and its register metadata
(vgpr_count, sgpr_count, the spill counts, private_segment_fixed_size, LDS and kernarg size) are.
Comments, .ident / .file lines and the compiler-version string are dropped; the function number in
basic-block labels (.LBB<fn>_<n>) is dropped too, since it only counts the functions above.

  git archive HEAD custom_op_benchmark_amd/csrc include | tar -x -C /tmp/parent
  python tools/kernel_diff.py /tmp/parent/custom_op_benchmark_amd/csrc custom_op_benchmark_amd/csrc \\
      gat_attention.hip gat_edge_attention.hip

No file list: every .hip file either side has.  A side's headers are <csrc>/../../include if that exists, else
this tree's.  Exit status 0 only if both sides have the same kernels and every one is identical.
"""
import collections
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAKEFILE = os.path.join(ROOT, "custom_op_benchmark_amd", "csrc", "Makefile")
META = (("vgpr_count", "vgpr"), ("sgpr_count", "sgpr"), ("vgpr_spill_count", "vspill"), ("sgpr_spill_count", "sspill"),
        ("private_segment_fixed_size", "scratch"), ("group_segment_fixed_size", "lds"),
        ("kernarg_segment_size", "kernarg"))


def _make_var(text, name):
    m = re.search(r"^%s\s*[?:]?=\s*((?:.*\\\n)*.*)$" % name, text, re.M)
    return m.group(1).replace("\\\n", " ")


def _command(csrc):
    """hipcc and the Makefile's CXXFLAGS with ROOT pointing at the side's own headers"""
    mk = open(MAKEFILE).read()
    inc = os.path.abspath(os.path.join(csrc, "..", ".."))
    if not os.path.isdir(os.path.join(inc, "include")):
        inc = ROOT
    flags = _make_var(mk, "CXXFLAGS").replace("$(ARCH)", _make_var(mk, "ARCH").strip()).replace("$(ROOT)", inc)
    return [os.environ.get("HIPCC", _make_var(mk, "HIPCC").strip())] + flags.split()


def _assemble(csrc, name, out):
    r = subprocess.run(_command(csrc) + ["--cuda-device-only", "-S", name, "-o", out], cwd=csrc,
                       capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("%s/%s does not compile:\n%s" % (csrc, name, r.stderr))
    return open(out).read()


def _kernels(asm):
    """-> {symbol: (instruction text, {metadata})} of one assembly file"""
    lines = asm.splitlines()
    meta, cur = {}, None
    for ln in lines:   # amdhsa.kernels: a list of maps whose keys sit two columns inside the dash
        m = re.match(r"^  (- | {2})\.(\w+):\s*(.*)$", ln)
        if not m:
            continue
        if m.group(1) == "- ":
            cur = {}
        if cur is not None:
            cur[m.group(2)] = m.group(3).strip().strip("'")
            if m.group(2) == "name":
                meta[cur["name"]] = cur
    label = {ln.split(":")[0]: n for n, ln in enumerate(lines) if re.match(r"^[A-Za-z_]\w*:", ln)}
    out = {}
    for sym, d in meta.items():
        body = []
        for ln in lines[label[sym] + 1:]:
            if re.match(r"^\.Lfunc_end\d+:", ln):
                break
            ln = ln.split(";")[0].rstrip()
            if not ln.strip() or re.match(r"\s*\.(ident|file)\b", ln) or "clang version" in ln:
                continue
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", ln))
        out[sym] = ("\n".join(body), {short: int(d.get(key, 0)) for key, short in META})
    return out


def _demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    return dict(zip(names, r.stdout.splitlines()))


def _template(dem):
    return re.sub(r"^void (graphop::)?", "", dem).split("<")[0].split("(")[0]


def _short(dem):
    return re.sub(r"\(.*$", "", re.sub(r"^void (graphop::)?", "", dem))


def _numbers(d):
    return " ".join("%s %d" % (short, d[short]) for _, short in META)


def main(argv):
    if len(argv) < 2:
        sys.exit(__doc__)
    sides = [os.path.abspath(argv[0]), os.path.abspath(argv[1])]
    files = argv[2:] or sorted({f for s in sides for f in os.listdir(s) if f.endswith(".hip")})
    tmp = tempfile.mkdtemp(prefix="kernel_diff_")
    jobs = {}
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(16, 2 * len(files))) as pool:
        for f in files:
            for n, s in enumerate(sides):
                if os.path.exists(os.path.join(s, f)):
                    jobs[(f, n)] = pool.submit(_assemble, s, f, os.path.join(tmp, "%d_%s.s" % (n, f)))
    bad = 0
    for f in files:
        a, b = (_kernels(jobs[(f, n)].result()) if (f, n) in jobs else {} for n in (0, 1))
        dem = _demangle(sorted(set(a) | set(b)))
        same, total = collections.Counter(), collections.Counter()
        differ, only = [], []
        for sym in sorted(dem, key=dem.get):
            t = _template(dem[sym])
            total[t] += 1
            if sym in a and sym in b:
                if a[sym] == b[sym]:
                    same[t] += 1
                else:
                    differ.append(sym)
            else:
                only.append(sym)
        print("%s: %d kernels in %s, %d in %s" % (f, len(a), argv[0], len(b), argv[1]))
        for t in sorted(total):
            print("  %-40s %3d / %3d identical" % (t, same[t], total[t]))
        for sym in differ:
            what = "instructions" if a[sym][0] != b[sym][0] else "metadata"
            print("  DIFFERS (%s): %s\n    %s\n    %s" % (what, _short(dem[sym]), _numbers(a[sym][1]),
                                                           _numbers(b[sym][1])))
        for sym in only:
            print("  ONLY IN %s: %s" % (argv[0] if sym in a else argv[1], _short(dem[sym])))
        bad += len(differ) + len(only)
    print("%s (assembly kept in %s)" % ("all kernels identical" if bad == 0 else "%d kernels differ" % bad, tmp))
    return 0 if bad == 0 else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
