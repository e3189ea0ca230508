"""Do the kernels of one .hip file keep their instructions across a change?  

    python scripts/compare_kernel_isa.py BEFORE.hip AFTER.hip [--arch gfx950]

Both files are compiled with the flags of dsmnet_amd/csrc/build.py plus ``-save-temps
-Rpass-analysis=kernel-resource-usage`` into two temporary directories (the include paths are this
tree's; BEFORE is typically ``git show REV:dsmnet_amd/csrc/NAME.hip > /tmp/before.hip``).  For
every kernel of BEFORE the script prints whether AFTER has a kernel of the same name -- a trailing
defaulted ``false`` template argument that the change added is ignored -- with the same instruction
text (label numbers apart), the same resource remarks (VGPR, SGPR, LDS, scratch, occupancy), and a
histogram of the opcodes of the lines that differ; then the kernels only AFTER has.  No GPU.
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REMARKS = (("TotalSGPRs", "SGPR"), ("VGPRs", "VGPR"), ("ScratchSize [bytes/lane]", "scratch"),
           ("LDS Size [bytes/block]", "LDS"), ("Occupancy [waves/SIMD]", "waves/SIMD"))


def compile_one(src, arch):
    out = tempfile.mkdtemp(prefix="isa_")
    name = os.path.join(out, "k.hip")
    with open(name, "w") as f:
        f.write(open(src).read())
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=" + arch, "-O3", "-std=c++17", "-fPIC",
           "-I" + os.path.join(ROOT, "dsmnet_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
           "-Rpass-analysis=kernel-resource-usage", "-save-temps", "-c", name, "-o", os.path.join(out, "k.o")]
    r = subprocess.run(cmd, cwd=out, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit("hipcc failed on %s:\n%s" % (src, r.stderr))
    asm = [f for f in os.listdir(out) if f.endswith(arch + ".s")]
    return os.path.join(out, asm[0]), r.stderr


def kernels(path):
    out, body = {}, None
    for l in open(path):
        m = re.match(r"^(_Z\w+):", l)
        if m:
            body = out.setdefault(m.group(1), [])
            continue
        if body is None:
            continue
        if l.startswith("\t.end_amdhsa_kernel") or l.startswith(".Lfunc_end"):
            body = None
            continue
        s = l.split(";")[0].strip()
        if s and not s.startswith("."):
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", s))
    return {k: v for k, v in out.items() if v}


def remarks(text):
    out, cur = {}, None
    for l in text.splitlines():
        m = re.search(r"Function Name: (\S+)", l)
        if m:
            cur = out.setdefault(m.group(1), {})
        for key, short in REMARKS:
            m = re.search(" " + re.escape(key) + r": (\d+)", l)
            if m and cur is not None:
                cur[short] = int(m.group(1))
    return out


def norm(name):
    """Drop one trailing ``false`` template argument (a defaulted parameter the change added)."""
    return re.sub(r"ELb0E(EEv)", r"E\1", name, count=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--arch", default="gfx950")
    args = ap.parse_args()
    (sa, ra), (sb, rb) = compile_one(args.before, args.arch), compile_one(args.after, args.arch)
    a, b = kernels(sa), kernels(sb)
    ra, rb = remarks(ra), remarks(rb)
    bn = {k: k for k in b}
    bn.update({norm(k): k for k in b if norm(k) not in b})
    hist, worst = collections.Counter(), 0
    for k in sorted(a):
        kb = bn.get(k)
        if kb is None:
            print("MISSING  ", k)
            worst = 1
            continue
        diff = [(x, y) for x, y in zip(a[k], b[kb]) if x != y]
        same_len, same_res = len(a[k]) == len(b[kb]), ra.get(k) == rb.get(kb)
        for x, y in diff:
            hist[(x.split()[0], y.split()[0])] += 1
        state = "same" if same_len and not diff else "%d lines differ" % len(diff) if same_len else "LENGTH %d -> %d" % (len(a[k]), len(b[kb]))
        if not same_len or not same_res:
            worst = 1
        print("%-18s remarks %-9s %s  %s" % (state, "same" if same_res else "DIFFER", ra.get(k), k))
    print("opcodes of the differing lines (before, after):", dict(hist))
    for k in sorted(b):
        if k not in bn.values() or all(bn.get(x) != k for x in a):
            print("NEW      ", rb.get(k), k)
    sys.exit(worst)


if __name__ == "__main__":
    main()
