"""What hipcc generates for one csrc/*.hip file (cross-compiled for gfx950, no GPU needed): the resource-usage remark of every
kernel and the assembly text, for the tests that hold kernels to register, scratch and occupancy targets."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CSRC = os.path.join(ROOT, "poseidon252_amd", "csrc")


def kernel_resources(hip_file, out):
    """compiles csrc/<hip_file> with the library's flags to the assembly file `out`; returns ({mangled kernel name: {vgpr, agpr,
    scratch, occ}} in the order of the file, the assembly text)"""
    from poseidon252_amd import build as b
    b._gen_assets()
    cmd = [b._hipcc()] + [f for f in b.HIPCC_FLAGS if f != "-fPIC"] + ["-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                                                                      "-o", str(out), os.path.join(CSRC, hip_file)]
    proc = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC)
    assert proc.returncode == 0, proc.stderr[-3000:]
    r = proc.stderr
    names = re.findall(r"Function Name: (\S+)", r)
    cols = [[int(x) for x in re.findall(pat, r)] for pat in (r"\bVGPRs: (\d+)", r"\bAGPRs: (\d+)", r"ScratchSize \[bytes/lane\]: (\d+)",
                                                               r"Occupancy \[waves/SIMD\]: (\d+)")]
    assert all(len(c) == len(names) for c in cols), r[-2000:]
    return {n: dict(zip(("vgpr", "agpr", "scratch", "occ"), vals)) for n, *vals in zip(names, *cols)}, open(out).read()
