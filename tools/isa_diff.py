#!/usr/bin/env python3
"""tools/isa_diff.py PARENT_CSRC THIS_CSRC [unit ...]: is the generated gfx950 code of two source trees the same?

Compiles the device side of every translation unit of build.UNITS (or of the units named) from both csrc folders with the
build's own flags plus `--cuda-device-only -S` and compares the assembly texts.  A host-only refactor must leave every unit
identical; the __hip_cuid_<hash of the source text> symbol is normalised.  A differing unit is listed with its first differing
lines.  A unit that only one tree has (a unit split off another, or merged into one) is listed with the kernels its assembly holds:
none for a host-only unit; otherwise the unit they moved from or to shows them missing or added in its own diff.  Exit status 0 = all
identical.  Both folders must sit in FULL trees (the sources include ../../include/orl_engine.h):
take the parent with `git worktree`, not with an archive of csrc alone.

    git worktree add /tmp/parent HEAD~1
    python tools/isa_diff.py /tmp/parent/offlinerl-kit_amd/csrc offlinerl-kit_amd/csrc
"""
import difflib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "offlinerl-kit_amd"))
import build  # noqa: E402


CUID = re.compile(r"__hip_cuid_[0-9a-f]+")      # per-unit symbol named after a hash of the SOURCE text: not code


def isa(csrc, unit, out):
    if not os.path.exists(os.path.join(csrc, unit)):
        return None
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc] + build.FLAGS + ["--cuda-device-only", "-S", os.path.join(csrc, unit), "-o", out])
    with open(out) as fh:
        return CUID.sub("__hip_cuid_X", fh.read()).splitlines()


def main():
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    a_dir, b_dir = sys.argv[1], sys.argv[2]
    units = sys.argv[3:] or list(build.UNITS)
    bad = 0
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=int(os.environ.get("MAX_JOBS", "8"))) as ex:
        jobs = {u: (ex.submit(isa, a_dir, u, os.path.join(tmp, "a_" + u + ".s")), ex.submit(isa, b_dir, u, os.path.join(tmp, "b_" + u + ".s")))
                for u in units}
        for u, (fa, fb) in jobs.items():
            a, b = fa.result(), fb.result()
            if a is None or b is None:
                have = a if b is None else b
                names = [x.split()[1] for x in have if x.strip().startswith(".amdhsa_kernel ")]
                print("%-22s only in the %s tree: %d kernels %s" % (u, "parent" if b is None else "new", len(names), " ".join(names)), flush=True)
                continue
            if a == b:
                print("%-22s identical (%d lines)" % (u, len(a)), flush=True)
                continue
            bad += 1
            d = [x for x in difflib.unified_diff(a, b, "parent/" + u, "this/" + u, lineterm="", n=0)]
            print("%-22s DIFFERS (%d / %d lines)" % (u, len(a), len(b)))
            print("\n".join(d[:40]), flush=True)
    print("%d of %d units differ" % (bad, len(units)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
