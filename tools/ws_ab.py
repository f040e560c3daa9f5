#!/usr/bin/env python3
"""tools/ws_ab.py: do two builds of the weight-stationary kernels (csrc/ws_*.hip) take the same instantiations and leave the same bits?

    ORL_ENGINE_LIB=<parent's library> python tools/ws_ab.py dump a.npz
    python tools/ws_ab.py dump b.npz                                        (fresh processes: one library per process)
    python tools/ws_ab.py cmp a.npz b.npz

``dump`` runs every launch of tests/ws_cases.py -- FLAVOURS, depth_cases() and geometry_cases(), the launches of tests/test_gpu_ws_paths.py --
through the unit tap (ws_cases.build / ws_cases.run) and stores, per launch, the tap's report (launcher, instantiation name and index, LDS
bytes, row groups) and the raw 32-bit words of every array as it comes back, results and operands.  After a launch that failed on the device
nothing more is launched (ws_cases.DEVICE_ERRORS).  ``dump FILE --dry-run`` stores the reports only and needs no GPU.  ``cmp`` lists each
differing key with its first differing index and exits non-zero on any difference."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "offlinerl-kit_amd")):      # as tests/conftest.py
    sys.path.insert(0, p)


def launches():
    import ws_cases as w
    out = [("flavour/" + name, kw) for name, kw in w.FLAVOURS.items()]
    out += [("depth/%s/M%d/per_z%d" % (name, M, pz), w.depth_kwargs(name, M, pz)) for name, M, pz in w.depth_cases()]
    out += [("geometry/%s/%s" % (label, name), w.geometry_kwargs(name, over)) for label, name, over in w.geometry_cases()]
    assert len(out) == len(set(k for k, _ in out))
    return out


def dump(path, dry_run):
    import ws_cases as w
    from offlinerlkit import _engine
    table = _engine.ws_flavours()
    out = {}
    for key, kw in launches():
        c = w.build(**kw)
        rep = w.run(c, dry_run=dry_run)      # raises, and refuses every later launch, after a device error
        out[key + "/report/flavour"] = np.asarray(table[rep["flavour_id"]])
        out[key + "/report"] = np.asarray([rep["launcher"], rep["flavour_id"], rep["lds"], rep["groups"]], np.int64)
        assert rep["flavour"] == table[rep["flavour_id"]]
        if not dry_run:
            for name, a in c.arrays.items():
                out[key + "/" + name] = a.raw.copy()
    np.savez_compressed(path, **out)
    arrays = [a for k, a in out.items() if "/report" not in k]
    print("ws_ab dump: %d launches, %d arrays, %d values -> %s" % (len(launches()), len(arrays), sum(a.size for a in arrays), path))


def cmp(pa, pb):
    a, b = np.load(pa), np.load(pb)
    bad = sorted(set(a.files) ^ set(b.files))
    for k in bad:
        print("%s: only in one file" % k)
    total = 0
    for k in sorted(set(a.files) & set(b.files)):
        x, y = a[k], b[k]
        total += x.size
        if x.shape != y.shape or x.dtype != y.dtype:
            print("%s: %s %s against %s %s" % (k, x.dtype, x.shape, y.dtype, y.shape))
            bad.append(k)
            continue
        ne = np.flatnonzero(x.ravel() != y.ravel())
        if ne.size:
            i = int(ne[0])
            print("%s: %d of %d differ, first at %d: %r against %r" % (k, ne.size, x.size, i, x.ravel()[i], y.ravel()[i]))
            bad.append(k)
    print("ws_ab cmp: %d keys, %d values compared (arrays as 32-bit words), %d keys differ" % (len(a.files), total, len(bad)))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) in (3, 4) and sys.argv[1] == "dump" and sys.argv[3:] in ([], ["--dry-run"]):
        dump(sys.argv[2], len(sys.argv) == 4)
    elif len(sys.argv) == 4 and sys.argv[1] == "cmp":
        sys.exit(cmp(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
