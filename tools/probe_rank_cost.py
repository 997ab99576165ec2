"""What the probes cost the rank stage (ANALYSIS TOOL).

    rocprofv3 --kernel-trace -d OUT -o run -- python tools/probe_rank_cost.py run \
        --workload complex-fb15k237-necessary --probes 8 [--steps 3]
    python tools/probe_rank_cost.py sum --batches 4 OUT/.../run_results.db [...]

``run`` evaluates bench.py's singleton batches of a workload one after the other on one
context (nothing overlaps, so a kernel's duration is its own) with ``--probes`` probes on
every slot: (s, p + i, o + 7 i + 1), facts nobody knows, so that every subject has as many
as asked for.  ``KELPIE_HIP_LIB`` selects the library, so a parent build (which knows no
probes: --probes 0) and this one alternate on one box.  ``sum`` adds up the trace of each run
as tools/topk_rank_cost.py does: the rank stage (the fp64 query kernels in both forms, the
filter bitmap, the kelpie column, kp_rank_f64_count), the attention, and everything, per
batch; ``--batches`` is the run's batch count (steps + 1: with probes the rank kernels are
launched once per chunk of probe rows as well, so their launches no longer count batches).
ConvE's probes also pass through the eval-mode encoder, which the slots' own rank rows share
kernels with: that part shows in ``device_us_per_batch`` only.
"""
import argparse
import json
import os
import sqlite3
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(a):
    import bench
    from kelpie_amd import NecessaryPostTrainingEngine
    wl = dict(bench.WORKLOADS[a.workload], _name=a.workload)
    assert wl["mode"] == "necessary"
    ds, model, _ = bench.build(wl, 0, 0)

    class Probed(NecessaryPostTrainingEngine):
        def _probes_of(self, pred):
            s, p, o = (int(v) for v in pred)
            if not a.probes:
                return None
            return (s, [(s, (p + i) % ds.num_relations, (o + 7 * i + 1) % ds.num_entities) for i in range(a.probes)])

    eng = Probed(model, ds, wl["hp"])
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
    print(json.dumps({"workload": a.workload, "probes": a.probes, "batches": a.steps + 1, "candidates": n,
                      "slots_last_batch": eng.last_batch_stats.get("slots"),
                      "probe_rows_last_batch": a.probes * (eng.last_batch_stats.get("slots") or 0)}))


RANK = ("kp_rank_filter_bits", "kp_rank_f64_kelpie", "kp_rank_f64_count", "rankq64")


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
        stage = sum(v[0] for v in rank.values())
        b = a.batches
        print(json.dumps({"db": db, "batches": b, "rank_launches_per_batch": round(rank["kp_rank_f64_kelpie"][1] / b, 2),
                          "rank_stage_us_per_batch": round(stage / b / 1e3, 1), "rank_share": round(stage / total, 4),
                          "attention_share": round(attn / total, 4), "device_us_per_batch": round(total / b / 1e3, 1),
                          "kernels_us_per_batch": {k: round(v[0] / b / 1e3, 1) for k, v in rank.items()}}))


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--workload", default="complex-fb15k237-necessary")
    r.add_argument("--probes", type=int, default=0)
    r.add_argument("--steps", type=int, default=3)
    s = sub.add_parser("sum")
    s.add_argument("--batches", type=int, required=True)
    s.add_argument("db", nargs="+")
    a = ap.parse_args()
    (run if a.cmd == "run" else summarise)(a)


if __name__ == "__main__":
    main()
