"""Writes tests/golden/pair_loop_parent.npz: what the plain tiled forces pass computed BEFORE it got its instantiation for a gravity
along z, for the four gravities of tests/pair_loop_cases.py.  Run it on a device, with the library of the commit that is to be the
reference (build that commit, or point SPHX_LIB at its libsphx.so):

    python tests/golden/make_pair_loop_golden.py [output.npz]

Per case the file holds the sha256 of the forces, position and velocity bytes after one pass and after 12 steps, the two time
steps, and every 16th row of each array (to see where and by how much a run differs when a digest does not match).
tests/test_gpu_pair_loop_bits.py demands equality with it."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(HERE, "..", ".."), os.path.join(HERE, "..")):
    sys.path.insert(0, os.path.abspath(p))

import pair_loop_cases as plc      # noqa: E402


def main(path):
    from gpusph_amd import capi
    lib = capi.load()
    has_entry = hasattr(lib, "sphx_dbg_forces_general_gravity")      # the reference commit has no such entry (ctypes looks it up here)
    rec = {}
    for case in plc.GRAVITIES:
        res = plc.run(case, force_general=True, path=has_entry)
        rec.update(plc.record(case, res))
        print("%-8s n=%d dt1=%.9g dt12=%.9g |f|max=%.6g" % (case, len(res["forces1"]), res["dt1"], res["dt12"],
                                                          np.abs(res["forces12"][:, :3]).max()))
    np.savez_compressed(path, **rec)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "pair_loop_parent.npz"))
