"""What the post-training trace costs (ANALYSIS TOOL).

    rocprofv3 --kernel-trace -d OUT -o run -- python tools/trace_cost.py run \
        --workload complex-fb15k237-necessary --trace 1 [--steps 3]
    python tools/trace_cost.py sum OUT/.../run_results.db [...]

``run`` evaluates bench.py's singleton batches of a workload one after the other on one
context (nothing overlaps, so a kernel's duration is its own) with ``engine.trace`` set or
not; ``KELPIE_HIP_LIB`` selects the library, so a parent build (which knows no trace:
--trace 0) and this one alternate on one box.  ``sum`` adds up the kernel trace of each run:
the device time per batch, the share of the kernels only a trace launches (the TRACE forms
of kp_cx_contrib and kp_te_posttrain count whole: they replace the plain forms; so does
kp_gemm_abt, which scores the ConvE trace's rows and also serves the encoder), and the
attention's share.
"""
import argparse
import json
import os
import sqlite3
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# kernels that only a trace launches
NEW = ("kp_cx_rowreg", "kp_cx_trace_sum", "kp_cv_trace_rows", "kp_cv_trace_row", "kp_cv_trace_slot")
# kernels with a TRACE form, and the GEMM the ConvE trace shares with the encoder (counted whole)
FORMS = ("kp_cx_contrib", "kp_te_posttrain", "kp_gemm_abt")


def run(a):
    import bench
    from kelpie_amd import NecessaryPostTrainingEngine
    wl = dict(bench.WORKLOADS[a.workload], _name=a.workload)
    assert wl["mode"] == "necessary"
    ds, model, _ = bench.build(wl, 0, 0)
    eng = NecessaryPostTrainingEngine(model, ds, wl["hp"])
    if a.trace:
        eng.trace = True
    per_step = wl.get("preds_per_step", 1)
    preds = bench.pick_preds(ds, (a.steps + 1) * per_step, seed=1234)
    bench.seed_all(42)
    n, steps, last = 0, 0, None
    for i in range(a.steps + 1):  # the first batch warms the context up; `sum` counts every batch alike
        items = [(p, [[c] for c in bench.candidates_of(ds, p, wl["candidates"])]) for p in
                 preds[i * per_step:(i + 1) * per_step]]
        eng.set_cache()
        out = eng.compute_relevance_multi(items)
        n += sum(len(o) for o in out)
        if a.trace:
            for res in eng.last_results:
                for side in (res if isinstance(res, tuple) else [s for pair in res for s in pair]):
                    steps += len(side.get("loss") or [])
                    last = (side.get("loss") or [last])[-1]
    print(json.dumps({"workload": a.workload, "trace": a.trace, "batches": a.steps + 1, "candidates": n,
                      "slots_last_batch": eng.last_batch_stats.get("slots"), "trace_values": steps,
                      "last_loss": last}))


def summarise(a):
    for db in a.db:
        rows = sqlite3.connect(db).execute("select name, start, end from kernels").fetchall()
        total = sum(e - s for _, s, e in rows)
        new = {k: sum(e - s for n, s, e in rows if k in n) for k in NEW}
        forms = {k: sum(e - s for n, s, e in rows if k in n) for k in FORMS}
        attn = sum(e - s for n, s, e in rows if "kp_attn" in n)
        batches = max(1, sum(1 for n, _, _ in rows if "kp_rank_f64_kelpie" in n))  # one launch per batch
        print(json.dumps({"db": db, "batches": batches, "device_us_per_batch": round(total / batches / 1e3, 1),
                          "new_kernels_share": round(sum(new.values()) / total, 5),
                          "attention_share": round(attn / total, 4),
                          "new_kernels_us_per_batch": {k: round(v / batches / 1e3, 1) for k, v in new.items()},
                          "form_kernels_us_per_batch": {k: round(v / batches / 1e3, 1) for k, v in forms.items()}}))


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--workload", default="complex-fb15k237-necessary")
    r.add_argument("--trace", type=int, default=0)
    r.add_argument("--steps", type=int, default=3)
    s = sub.add_parser("sum")
    s.add_argument("db", nargs="+")
    a = ap.parse_args()
    (run if a.cmd == "run" else summarise)(a)


if __name__ == "__main__":
    main()
