"""Resource figures of every kernel of one or more csrc/*.hip files, from the compiler's own remarks:

    python scripts/kernel_resources.py attention3.hip rowops.hip uvit.hip            # a markdown table per file
    python scripts/kernel_resources.py --against <other checkout> attention3.hip     # ... and the kernels whose figures differ there

Compiles with the Makefile's flags plus -Rpass-analysis=kernel-resource-usage (no GPU needed) and prints SGPRs, VGPRs, AGPRs, scratch bytes
per lane, LDS bytes per block and occupancy per kernel (demangled).  profiles/uvit_dropout.md's tables are this output; regenerate them after
a ROCm update - the DROP kernels of attention3.hip stay free of scratch only because of how their loops are unrolled."""
import argparse
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("SGPRs", "VGPRs", "AGPRs", "ScratchSize", "LDS", "Occupancy")


def figures(root, src, hipcc):
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result", "-Rpass-analysis=kernel-resource-usage",
                        "-c", src, "-o", os.devnull], cwd=os.path.join(root, "open-muse_amd", "csrc"), capture_output=True, text=True)
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: (.*)$", line)
        if not m:
            continue
        t = m.group(1).strip()
        m2 = re.match(r"Function Name: (\S+)", t)
        if m2:
            cur = m2.group(1)
            out[cur] = {}
            continue
        m3 = re.search(r"(SGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", t)
        if m3 and cur:
            out[cur][m3.group(1).split(" ")[0]] = int(m3.group(2))
    if r.returncode:
        raise SystemExit(r.stderr[-2000:])
    return out


def demangle(names):
    try:
        return dict(zip(names, subprocess.run(["c++filt"] + list(names), capture_output=True, text=True, check=True).stdout.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("sources", nargs="+")
    ap.add_argument("--against", help="another checkout of the repository to compare with, kernel by kernel (mangled names)")
    ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    a = ap.parse_args()
    for src in a.sources:
        new = figures(ROOT, src, a.hipcc)
        names = demangle(list(new))
        print(f"### {src}: {len(new)} kernels, {sum(1 for v in new.values() if v.get('ScratchSize'))} with scratch\n")
        print("| kernel | " + " | ".join(KEYS) + " |\n|---|" + "---|" * len(KEYS))
        for k, v in new.items():
            print(f"| `{names[k]}` | " + " | ".join(str(v.get(x, "")) for x in KEYS) + " |")
        if a.against:
            old = figures(a.against, src, a.hipcc)
            diff = [k for k in old if old[k] != new.get(k)]
            print(f"\nagainst {a.against}: {len(old)} kernels there; figures differ (or the kernel is gone) for: {diff or 'none'}")
        print()
