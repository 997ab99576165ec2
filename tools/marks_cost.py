"""What the epoch marks cost (ANALYSIS TOOL).

    rocprofv3 --kernel-trace -d OUT -o run -- python tools/marks_cost.py run \
        --workload complex-fb15k237-sufficient --marks 4 [--steps 3]
    python tools/marks_cost.py sum OUT/.../run_results.db [...]

``run`` evaluates bench.py's singleton batches of a workload one after the other on one
context (nothing overlaps, so a kernel's duration is its own) with ``engine.marks`` set to
``--marks`` epochs spread evenly over the post-training and ending at its last epoch (0: no
marks).  ``sum`` adds up the kernel trace of each run: the device time per batch, the rank
stage (the fp64 query kernels, the filter bitmaps, the kelpie column and kp_rank_f64_count:
with marks it ranks n more rows per slot), the update kernels (their MARKS form stores the
rows) and, for ConvE, the eval-mode encoder the mark rows pass through.
"""
import argparse
import json
import os
import sqlite3
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RANK = ("kp_rank_filter_bits", "kp_rank_f64_kelpie", "kp_rank_f64_count", "rankq64")
UPDATE = ("kp_cx_update", "kp_cv_update", "kp_te_posttrain")
ENCODER = ("kp_cv_conv_fwd", "kp_gemm_abt", "kp_cv_post_fc")  # shared with the step loop's unfused paths


def mark_epochs(n, epochs):
    """n distinct epochs in [1, epochs] ending at ``epochs``, evenly spread."""
    return sorted({max(1, round(epochs * (j + 1) / n)) for j in range(n)})


def run(a):
    import bench
    from kelpie_amd import NecessaryPostTrainingEngine, SufficientPostTrainingEngine
    wl = dict(bench.WORKLOADS[a.workload], _name=a.workload)
    ds, model, _ = bench.build(wl, 0, 0)
    suff = wl["mode"] == "sufficient"
    eng = (SufficientPostTrainingEngine if suff else NecessaryPostTrainingEngine)(model, ds, wl["hp"])
    marks = mark_epochs(a.marks, int(wl["hp"]["epochs"])) if a.marks else None
    eng.marks = marks
    per_step = wl.get("preds_per_step", 1)
    preds = bench.pick_preds(ds, (a.steps + 1) * per_step, seed=1234)
    bench.seed_all(42)
    jobs = []
    for i in range(a.steps + 1):
        step = []
        for p in preds[i * per_step:(i + 1) * per_step]:
            cands = [[c] for c in bench.candidates_of(ds, p, wl["candidates"])]
            if suff:
                ents = eng.select_entities_to_convert(p, wl["convert"], 200)
                if ents:
                    step.append((p, cands, ents))
            else:
                step.append((p, cands))
        jobs.append(step)
    n = n_marks = 0
    for items in jobs:  # the first batch warms the context up; `sum` counts every batch alike
        eng.set_cache()
        out = eng.compute_relevance_multi(items)
        n += sum(len(o) for o in out)
        n_marks += (eng.last_batch_stats.get("slots") or 0) * len(marks or [])
    print(json.dumps({"workload": a.workload, "marks": marks, "batches": a.steps + 1, "candidates": n,
                      "slots_last_batch": eng.last_batch_stats.get("slots"), "mark_rows": n_marks}))


def summarise(a):
    for db in a.db:
        rows = sqlite3.connect(db).execute("select name, start, end from kernels").fetchall()
        total = sum(e - s for _, s, e in rows)

        def group(keys):
            return {k: sum(e - s for n, s, e in rows if k in n) for k in keys}

        rank, upd, enc = group(RANK), group(UPDATE), group(ENCODER)
        attn = sum(e - s for n, s, e in rows if "kp_attn" in n)
        # the slots' own rank launches kp_rank_f64_kelpie once per batch; the marks' chunks add theirs
        batches = max(1, a.batches or sum(1 for n, _, _ in rows if "kp_rank_f64_kelpie" in n))
        us = lambda v: round(v / batches / 1e3, 1)  # noqa: E731
        print(json.dumps({"db": db, "batches": batches, "device_us_per_batch": us(total),
                          "rank_stage_us_per_batch": us(sum(rank.values())), "attention_share": round(attn / total, 4),
                          "rank_us_per_batch": {k: us(v) for k, v in rank.items()},
                          "update_us_per_batch": {k: us(v) for k, v in upd.items() if v},
                          "encoder_us_per_batch": {k: us(v) for k, v in enc.items() if v}}))


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--workload", default="complex-fb15k237-sufficient")
    r.add_argument("--marks", type=int, default=0)
    r.add_argument("--steps", type=int, default=3)
    s = sub.add_parser("sum")
    s.add_argument("--batches", type=int, default=0, help="batches of the run (0: count the slots' rank launches)")
    s.add_argument("db", nargs="+")
    a = ap.parse_args()
    (run if a.cmd == "run" else summarise)(a)


if __name__ == "__main__":
    main()
