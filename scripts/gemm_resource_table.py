"""Compiled-resource table of the decode GEMM kernels, from the compiler's own kernel-resource-usage remarks.

    python scripts/gemm_resource_table.py [CSRC_KERNELS_DIR] > table.txt

Compiles the six decode-GEMM files for the device only, with the package's kernel flags, and prints one line per
kernel (sorted): kernel<template arguments>, VGPRs, AGPRs, SGPRs, scratch bytes per lane, occupancy (waves per SIMD),
LDS bytes per block; a file's decode kernel is named by the file (gemm, z12, fp8, fp4, fp8a, q4).  Two tables (two trees)
are compared with diff; no GPU is needed.
"""
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
from llm_based_apache_spark_optimization_amd.ops.build import ARCH, HIPCC  # noqa: E402

FILES = ["gemm", "gemm_z12", "gemm_fp8", "gemm_fp4", "gemm_fp8a", "gemm_q4"]
FLAGS = [f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=fast", "-Wno-unused-result"]
KEYS = {"VGPRs": "vgpr", "AGPRs": "agpr", "TotalSGPRs": "sgpr", "ScratchSize [bytes/lane]": "scratch",
        "Occupancy [waves/SIMD]": "occ", "LDS Size [bytes/block]": "lds"}


def short(sym: str, stem: str = "") -> str:
    """_Z<n><name>I<Li1E|Lb0E ...>E... -> name<1,0,...>: the template arguments identify a kernel of one file."""
    m = re.match(r"_Z(\d+)", sym)
    if not m:
        return sym
    name, rest = sym[m.end():m.end() + int(m.group(1))], sym[m.end() + int(m.group(1)):]
    a = re.match(r"I((?:L[a-z]\d+E)+)E", rest)
    if name.endswith("skinny_kernel") or name == "gemm_z12_kernel":
        name = stem.replace("gemm_", "")
    return name + ("<" + ",".join(re.findall(r"L[a-z](\d+)E", a.group(1))) + ">" if a else "")


def table(kdir: Path, stem: str) -> list[str]:
    r = subprocess.run([HIPCC, *FLAGS, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                        str(kdir / f"{stem}.hip"), "-o", "/dev/null"], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-4000:])
    rows, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(.+?): (\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        k, v = m.group(1).strip(), m.group(2)
        if k == "Function Name":
            cur = rows.setdefault(v, {})
        elif cur is not None and k in KEYS:
            cur[KEYS[k]] = v
    lines = {short(sym, stem): f"{short(sym, stem)} {d['vgpr']} {d['agpr']} {d['sgpr']} {d['scratch']} {d['occ']} {d['lds']}"
             for sym, d in rows.items()}
    assert len(lines) == len(rows), "two kernels share a short name"
    return [lines[k] for k in sorted(lines)]


def main() -> None:
    kdir = Path(sys.argv[1]) if len(sys.argv) > 1 else REPO / "csrc" / "kernels"
    print("# kernel<template arguments> VGPRs AGPRs SGPRs scratch occupancy LDS")
    with ThreadPoolExecutor(max_workers=len(FILES)) as ex:
        for stem, lines in zip(FILES, ex.map(lambda s: table(kdir, s), FILES)):
            print(f"# {stem}: {len(lines)} kernels")
            print("\n".join(lines))


if __name__ == "__main__":
    main()
