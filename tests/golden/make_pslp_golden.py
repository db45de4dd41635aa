"""Generates tests/golden/pslp_reference.json: what the presolver the reference vendors (PSLP v0.0.8) makes of the LPs of
tests/test_presolve.py's comparison tests -- its status, the size of its reduced model and its postsolve of the reduced model's
exact optimum (HiGHS via scipy), back in the original dimensions.  The tests compare our presolve with these records, so they
run without PSLP.
Run (PSLP built into oracle/_ref/ first: make -C oracle refpslp):  python tests/golden/make_pslp_golden.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from test_presolve import doubleton_lp, highs, structured_lp  # noqa: E402

from oracle import pslp_ref  # noqa: E402

CASES = [("structured_%d" % s, lambda s=s: structured_lp(s)) for s in (1, 2, 3)] + \
        [("doubleton_%d_%g" % (s, f), lambda s=s, f=f: doubleton_lp(s, free_share=f)) for s, f in ((31, 0.0), (34, 0.0), (42, 0.5), (43, 0.5))]


def record(lp):
    ref = pslp_ref.RefPresolve(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"], lp["c"])
    out = {"m": lp["m"], "n": lp["n"], "nnz": len(lp["values"]), "status": ref.status, "rm": ref.rm, "rn": ref.rn, "x": None, "y": None, "z": None}
    if ref.rm > 0 and ref.rn > 0:
        _, xr, yr, zr = highs(ref.rm, ref.rn, ref.Ap, ref.Ai, ref.Ax, ref.lhs, ref.rhs, ref.lbs, ref.ubs, ref.c)
    else:
        xr, yr, zr = np.zeros(ref.rn), np.zeros(ref.rm), np.zeros(ref.rn)
    out["x"], out["y"], out["z"] = ([float(v) for v in a] for a in ref.postsolve(xr, yr, zr))
    ref.close()
    return out


if __name__ == "__main__":
    if not pslp_ref.available():
        raise SystemExit("oracle/_ref/libpslp_ref.so is not built (make -C oracle refpslp)")
    recs = {key: record(make()) for key, make in CASES}
    json.dump(recs, open(os.path.join(HERE, "pslp_reference.json"), "w"), indent=0)
    for key, r in recs.items():
        print(key, r["m"], "x", r["n"], "-> PSLP", r["rm"], "x", r["rn"], "status", r["status"])
