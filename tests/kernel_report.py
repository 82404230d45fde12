"""The compiler's resource report of the gfx950 kernels of one file of csrc/src/kernels: what the
native tests assert on (kernel names, scratch, spills, LDS) and what an A/B of two builds compares
(registers, occupancy, code bytes). A plain module: import it, it is neither a fixture file nor a
conftest."""
import os
import re
import subprocess
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"

# record key -> the label of its line in a -Rpass-analysis=kernel-resource-usage remark
FIELDS = {"vgprs": "VGPRs", "agprs": "AGPRs", "sgprs": "SGPRs", "scratch": r"ScratchSize \[bytes/lane\]",
          "vgpr_spills": "VGPRs Spill", "sgpr_spills": "SGPRs Spill", "lds": r"LDS Size \[bytes/block\]",
          "occupancy": r"Occupancy \[waves/SIMD\]"}


class KernelReport(list):
    """One dict per kernel, in the compiler's order: `name` (mangled) and the keys of FIELDS.
    `asm`: the device assembly (emit="asm"); emit="obj" adds `code_bytes` to every record."""
    asm = ""

    def column(self, key):
        return [k[key] for k in self]


def kernel_report(src, emit=None, repo=REPO):
    """Compile csrc/src/kernels/<src> of `repo` for gfx950 and return its KernelReport.
    emit: None (host and device, nothing kept), "asm" or "obj" (device only)."""
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{repo}/csrc/include"]
    with tempfile.TemporaryDirectory() as tmp:
        obj = os.path.join(tmp, "k.o")
        cmd += {None: ["-c", "-o", os.devnull], "asm": ["-S", "--cuda-device-only", "-o", "-"],
                "obj": ["-c", "--cuda-device-only", "--no-gpu-bundle-output", "-o", obj]}[emit]
        r = subprocess.run(cmd + [f"{repo}/csrc/src/kernels/{src}", "-Rpass-analysis=kernel-resource-usage"],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        sizes = {}
        if emit == "obj":
            syms = subprocess.run([READELF, "-sW", obj], capture_output=True, text=True, check=True).stdout
            sizes = {m[1]: int(m[0]) for m in re.findall(r"^\s*\d+:\s+\w+\s+(\d+)\s+FUNC\s.*\s(\S+)$", syms, re.M)}
    report = KernelReport()
    report.asm = r.stdout if emit == "asm" else ""
    for block in r.stderr.split("Function Name: ")[1:]:
        rec = {"name": block.split()[0]}
        for key, label in FIELDS.items():
            rec[key] = int(re.search(label + r": (\d+)", block).group(1))
        if sizes:
            rec["code_bytes"] = sizes[rec["name"]]
        report.append(rec)
    return report
