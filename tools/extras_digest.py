"""Digests of one post-training call with every optional request on, per model family.

    python tools/extras_digest.py [> profiles/<dir>/digest_<build>.txt]

For marks_cases' four family cases (the ones tests/test_marks_gpu.py calls FAMILY) the first
engine batch runs again directly with topk = 5, seven probes per slot, the trace, the case's
marks and the margins at tol = 1e-4; one sha256 per output is printed (one per margin array of
the slots, the probes and the marks), then the median ``last_timing()["device_s"]``
of five repeats after one warm-up.  Then, for kp_posttrain_rank_f64, one sha256 per case of
f64_cases.ALL over every slot's fp64 score, rank and row.  Only ``Context.posttrain_rank``'s
public keywords, ``marks_cases.run`` and ``f64_cases.run`` are used, so the same file runs on an
older checkout: two builds compute the same bits exactly when their lines are equal
(KELPIE_HIP_LIB selects the library).
"""
import hashlib
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import marks_cases as mc  # noqa: E402

FAMILY = ("ComplEx-d32-DB4", "DistMult-d40-DB4", "ConvE-d60-DB4", "TransE-d16-VPL1-NT1024")
PROBES_PER_SLOT = 7


def probes_of(args, n_ent, per_slot=PROBES_PER_SLOT):
    """``per_slot`` probes for every slot: the slot's relation towards its own object and the
    next ids; the first carries the slot's filter list, the others none."""
    _, _, row_off, _, _, _, pred, filt_off, filt = args
    n = len(row_off) - 1
    trip, f_off, f = [], [0], []
    for i in range(n):
        for j in range(per_slot):
            trip.append((int(pred[i][1]), (int(pred[i][2]) + 3 * j) % n_ent))
            if j == 0:
                f.extend(int(v) for v in filt[filt_off[i]:filt_off[i + 1]])
            f_off.append(len(f))
    return (np.arange(n + 1, dtype=np.int32) * per_slot, np.asarray(trip, np.int32), np.asarray(f_off, np.int32),
            np.asarray(f, np.int32))


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def main():
    for case in (c for c in mc.CASES if c["id"] in FAMILY):
        batches, model = mc.run(case, lambda m: m.ctx)
        ctx = model.ctx._ctx  # (model.ctx is marks_cases.Capture around the device's)
        args = batches[0]["args"]
        kw = {"topk": 5, "probes": probes_of(args, ctx.n_ent), "trace": True, "marks": mc.marks_of(case),
              "margins": 1e-4}

        def call():
            return ctx.posttrain_rank(*args, want_x=True, **kw)

        s, r, x, (ids, top), (ps, pr), losses, (ms, mr, mx), margins = call()
        for name, arrays in (("score", (s,)), ("rank", (r,)), ("rows", (x,)), ("list_ids", (ids,)),
                             ("list_scores", (top,)), ("probe_score", (ps,)), ("probe_rank", (pr,)),
                             ("losses", losses), ("mark_score", (ms,)), ("mark_rank", (mr,)), ("mark_rows", (mx,))):
            print(f"{case['id']} {name} {sha(*arrays)}")
        for kind, fields in zip(("slots", "probes", "marks"), margins):
            for field in sorted(fields):
                print(f"{case['id']} margin_{kind}_{field} {sha(fields[field])}")
        times = []
        for _ in range(5):
            call()
            times.append(ctx.last_timing()["device_s"])
        print(f"{case['id']} device_s_median {statistics.median(times):.6e}")
    fp64_block()


def fp64_block():
    """kp_posttrain_rank_f64: for every case of f64_cases.ALL one sha256 over every recorded
    slot's fp64 score, rank and row, through a recording wrapper of the device's context as
    tests/test_f64_gpu.py runs them (the forced key ranges under KP_ATTN_RANGES)."""
    import f64_cases as fc
    from f64_backend import F64Recording

    for case in fc.ALL:
        if "ranges" in case:
            os.environ["KP_ATTN_RANGES"] = str(case["ranges"])  # read when the context is created
        try:
            slots = fc.run(case, lambda m: F64Recording(m.ctx))
        finally:
            os.environ.pop("KP_ATTN_RANGES", None)
        digest = sha(*(a for s in slots for a in (np.float64(s["score"]), np.int64(s["rank"]), s["x"])))
        print(f"fp64 {case['id']} slots {len(slots)} {digest}")


if __name__ == "__main__":
    main()
