"""What the compiler made of every kernel of one or more csrc/*.hip files, as a table that two checkouts can be compared by:

    python scripts/kernel_digest.py gemm.hip gemm_p.hip                  # a markdown table per file
    python scripts/kernel_digest.py --root <other checkout> gemm.hip     # ... of another checkout of the repository

Compiles to gfx950 assembly with the Makefile's flags (CXXFLAGS and the file's FLAGS_<name>) plus --cuda-device-only -S (no GPU needed) and
prints per kernel (demangled): instructions, VGPRs, SGPRs, scratch bytes per lane, occupancy, and a digest of the instruction stream - comments
and directives dropped, the function number of local labels (.LBB<n>_) normalised - so that a refactor which only moves inlined code between
templates can show that every kernel came out the same, instruction for instruction.  The second digest ("body") is that of the stream from
the first local label to the end: a kernel whose set-up code before its first branch target was merely reordered shows the same body (a
kernel without a label has one digest).  profiles/gemm256_refactor_isa.md and profiles/glu_refactor_isa.md are this output."""
import argparse
import hashlib
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INFO = {"NumVgprs": "vgprs", "NumSgprs": "sgprs", "TotalNumSgprs": "sgprs", "ScratchSize": "scratch", "Occupancy": "occupancy"}


def parse(asm):
    """-> [{name (mangled), insts, vgprs, sgprs, scratch, occupancy, digest, body}] for every kernel (.amdhsa_kernel) of an assembly listing"""
    funcs, kernels, cur, last, info = {}, [], None, None, None
    for raw in asm.splitlines():
        m = re.match(r";\s*(\w+):\s*(\d+)\s*$", raw.strip())
        if info is not None and m and m.group(1) in INFO:
            info.setdefault(INFO[m.group(1)], int(m.group(2)))
        line = raw.split(";", 1)[0].strip()
        if raw.strip().startswith("; Kernel info:"):
            info = last
        elif re.match(r"\.Lfunc_end\d+:", line):
            last, cur = cur, None
        elif re.match(r"\.amdhsa_kernel\s", line):
            kernels.append(line.split()[1])
        elif re.match(r"[A-Za-z_$][\w$.]*:$", line) and cur is None:
            cur = funcs[line[:-1]] = {"name": line[:-1], "stream": []}
            info = None
        elif cur is not None and line and (not line.startswith(".") or line.startswith(".LBB")):
            cur["stream"].append(re.sub(r"\.LBB\d+_", ".LBB_", " ".join(line.split())))
    out = []
    for k in kernels:
        f = funcs[k]
        stream = f.pop("stream")
        f["insts"] = sum(1 for s in stream if not s.endswith(":"))
        first = next((i for i, s in enumerate(stream) if s.startswith(".LBB") and s.endswith(":")), 0)
        f["digest"], f["body"] = (hashlib.sha256("\n".join(part).encode()).hexdigest()[:16] for part in (stream, stream[first:]))
        out.append(f)
    return out


def flags(root, src):
    mk = open(os.path.join(root, "open-muse_amd", "csrc", "Makefile")).read()
    var = lambda name: (re.search(rf"^{name}\s*\??=\s*(.*)$", mk, re.M) or [None, ""])[1]
    return (var("CXXFLAGS").replace("$(ARCH)", var("ARCH")) + " " + var("FLAGS_" + os.path.splitext(os.path.basename(src))[0])).split()


def demangle(names):
    try:
        return dict(zip(names, subprocess.run(["c++filt"] + list(names), capture_output=True, text=True, check=True).stdout.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("sources", nargs="+")
    ap.add_argument("--root", default=ROOT, help="the checkout to compile (default: this one)")
    ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    ap.add_argument("--flag", action="append", default=[], help="a further compiler flag, e.g. --flag=-DG256_TIMESTAMPS")
    a = ap.parse_args()
    for src in a.sources:
        r = subprocess.run([a.hipcc] + flags(a.root, src) + a.flag + ["--cuda-device-only", "-S", src, "-o", "-"],
                           cwd=os.path.join(a.root, "open-muse_amd", "csrc"), capture_output=True, text=True)
        if r.returncode:
            raise SystemExit(r.stderr[-2000:])
        ks = parse(r.stdout)
        names = demangle([k["name"] for k in ks])
        print(f"### {src}: {len(ks)} kernels\n\n| kernel | insts | VGPRs | SGPRs | scratch | occupancy | digest | body |\n|---|---|---|---|---|---|---|---|")
        for k in sorted(ks, key=lambda k: names[k["name"]]):
            print(f"| `{names[k['name']]}` | {k['insts']} | {k.get('vgprs')} | {k.get('sgprs')} | {k.get('scratch')} | {k.get('occupancy')} | {k['digest']} | {k['body']} |")
        print()
