"""Proof of coverage for tests/test_gpu_kernel_matrix.py: the in-scope kernel instantiations (tests/kernel_matrix.py: the seven
step / rollout families and the four A-templated operator families) of the built library that a rocprofv3 run never launched.

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o km -- python -m pytest -m gpu tests/test_gpu_kernel_matrix.py
    python scripts/kernel_coverage.py <dir> [library]

Reads every *kernel_stats.csv (else *kernel_trace.csv) under <dir>, takes the library's kernel list from isa_audit.disassemble,
demangles both the same way and prints the launched / built counts per family and every unreached instantiation.  Exit status 1
when any in-scope instantiation was never launched (or a launched name is not in the library)."""
import csv
import glob
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import kernel_matrix as km  # noqa: E402


def traced_names(trace_dir):
    """the kernel names of a rocprofv3 csv run (the stats file has one row per kernel; the trace one per dispatch)"""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True)
    col = "Name"
    if not files:
        files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
        col = "Kernel_Name"
    if not files:
        raise SystemExit(f"{trace_dir}: no rocprofv3 kernel_stats.csv / kernel_trace.csv")
    names = set()
    for f in files:
        with open(f, newline="") as fh:
            for row in csv.DictReader(fh):
                names.add(row[col])
    return sorted(names)


def main(argv):
    if not argv:
        print(__doc__)
        return 2
    lib = argv[1] if len(argv) > 1 else os.path.join(ROOT, "torchdriveenv_amd", "libtde_hip.so")
    with tempfile.TemporaryDirectory() as d:
        built = km.library_labels(lib, d)
    launched = {lb for lb in map(km.label_of, km.demangle(traced_names(argv[0]))) if km.in_scope(lb)}
    missing, foreign = sorted(built - launched), sorted(launched - built)
    print(f"library: {os.path.relpath(lib, ROOT)}")
    print(f"in-scope instantiations: {len(built)} built, {len(built & launched)} launched, {len(missing)} never launched")
    for fam in km.FAMILIES:
        b = {lb for lb in built if lb.split("<")[0] == fam}
        print(f"  {fam:26s} {len(b & launched):4d} / {len(b):4d}")
    for lb in missing:
        print(f"NOT LAUNCHED: {lb}")
    for lb in foreign:
        print(f"LAUNCHED BUT NOT IN THE LIBRARY: {lb}")
    return 1 if (missing or foreign) else 0


if __name__ == "__main__":
    raise SystemExit(main(sys.argv[1:]))
