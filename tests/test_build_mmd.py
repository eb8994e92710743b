"""CPU: the compiled form of csrc/mmd.hip (hipcc cross-compiles gfx950 without a GPU) - resource usage only."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_mmd_kernels_compile_without_scratch(tmp_path):
    """the pair-sum kernel keeps a 16 x 64 strip of f64 dot products in registers, indexed by unrolled loops, next to five running squared
    norms and two steps of five float4 loads: an index the compiler could not resolve would move them to scratch memory, and the kernel would still
    give the right bits, many times slower.  Every kernel of the file compiles with ScratchSize 0, with the Makefile's flags."""
    src = os.path.join(ROOT, "open-muse_amd", "csrc", "mmd.hip")
    mk = open(os.path.join(ROOT, "open-muse_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bmmd\.hip\b", mk, flags=re.M), "mmd.hip is not in the Makefile's SRCS"
    own = re.search(r"^FLAGS_mmd\s*=\s*(.*)$", mk, flags=re.M)
    flags = own.group(1).split() if own else []
    cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result"] + flags + \
          ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "mmd.o")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", r.stderr, flags=re.S)
    names = " ".join(name for name, _ in kernels)
    for wanted in ("row_norms_f64_kernel", "rbf_pair_sums_kernelILb0", "rbf_pair_sums_kernelILb1", "rbf_finalize_kernel"):
        assert wanted in names, (wanted, names)
    for name, scratch in kernels:
        assert int(scratch) == 0, (name, scratch)
