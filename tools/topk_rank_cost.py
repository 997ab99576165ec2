"""What the top-k selection costs the rank stage (ANALYSIS TOOL).

    rocprofv3 --kernel-trace -d OUT -o run -- python tools/topk_rank_cost.py run \
        --workload complex-fb15k237-necessary --topk 5 [--steps 3]
    python tools/topk_rank_cost.py sum OUT/.../run_results.db [...]

``run`` evaluates bench.py's singleton batches of a workload one after the other on one
context (nothing overlaps, so a kernel's duration is its own) with ``engine.top_k`` set;
``KELPIE_HIP_LIB`` selects the library, so a parent build (which knows no lists: --topk 0)
and this one alternate on one box.  ``sum`` adds up the trace of each run: the rank stage
(the fp64 query kernels, the filter bitmap, the kelpie column, kp_rank_f64_count and the
list merge; the table transpose, built once per context, is left out), the attention, and
everything, per batch.
"""
import argparse
import json
import os
import sqlite3
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RANK = ("kp_rank_filter_bits", "kp_rank_f64_kelpie", "kp_rank_f64_count", "kp_rank_topk_merge", "rankq64")


def run(a):
    import bench
    from kelpie_amd import NecessaryPostTrainingEngine
    wl = dict(bench.WORKLOADS[a.workload], _name=a.workload)
    assert wl["mode"] == "necessary"
    ds, model, _ = bench.build(wl, 0, 0)
    eng = NecessaryPostTrainingEngine(model, ds, wl["hp"])
    eng.top_k = a.topk
    per_step = wl.get("preds_per_step", 1)
    preds = bench.pick_preds(ds, (a.steps + 1) * per_step, seed=1234)
    bench.seed_all(42)
    n = 0
    for i in range(a.steps + 1):  # the first batch warms the context up; `sum` counts every batch alike
        items = [(p, [[c] for c in bench.candidates_of(ds, p, wl["candidates"])]) for p in
                 preds[i * per_step:(i + 1) * per_step]]
        eng.set_cache()
        out = eng.compute_relevance_multi(items)
        n += sum(len(o) for o in out)
    print(json.dumps({"workload": a.workload, "topk": a.topk, "batches": a.steps + 1, "candidates": n,
                      "slots_last_batch": eng.last_batch_stats.get("slots")}))


def summarise(a):
    for db in a.db:
        rows = sqlite3.connect(db).execute("select name, start, end from kernels").fetchall()
        total = sum(e - s for _, s, e in rows)
        rank = {k: [0, 0] for k in RANK}
        for n, s, e in rows:
            for k in RANK:
                if k in n:
                    rank[k][0] += e - s
                    rank[k][1] += 1
                    break
        attn = sum(e - s for n, s, e in rows if "kp_attn" in n)
        batches = max(1, rank["kp_rank_f64_kelpie"][1])  # one launch per batch
        stage = sum(v[0] for v in rank.values())
        print(json.dumps({"db": db, "batches": batches, "rank_stage_us_per_batch": round(stage / batches / 1e3, 1),
                          "rank_share": round(stage / total, 4), "attention_share": round(attn / total, 4),
                          "device_us_per_batch": round(total / batches / 1e3, 1),
                          "kernels_us_per_batch": {k: round(v[0] / batches / 1e3, 1) for k, v in rank.items()}}))


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--workload", default="complex-fb15k237-necessary")
    r.add_argument("--topk", type=int, default=0)
    r.add_argument("--steps", type=int, default=3)
    s = sub.add_parser("sum")
    s.add_argument("db", nargs="+")
    a = ap.parse_args()
    (run if a.cmd == "run" else summarise)(a)


if __name__ == "__main__":
    main()
