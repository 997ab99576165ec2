"""What keyed draws cost and save (ANALYSIS TOOL).

    python tools/keyed_cost.py run --workload transe-fb15k237-necessary [--pairs 3] [--steps 6]
    rocprofv3 --kernel-trace -d OUT -o run -- python tools/keyed_cost.py run \
        --workload transe-fb15k237-necessary --pairs 1 --modes keyed
    python tools/keyed_cost.py sum OUT/.../run_results.db [...]

``run`` evaluates bench.py's singleton batches of a workload one after the other on one
context, ``--pairs`` times in reference mode and in keyed mode alternately (one warm-up batch
per leg, not counted), and prints one JSON line per leg: candidates per second, the host time
of scheduling (in reference mode: the draws and the wait for them), of packing and of the
library call per batch, and the bytes of x0 and draws a batch hands the library (keyed: the two
keys per slot).  ``sum`` adds up the generation kernels (kp_key_x0, kp_key_perm, kp_key_words)
of a kernel trace against the whole trace.
"""
import argparse
import json
import os
import sqlite3
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEYED = ("kp_key_x0", "kp_key_perm", "kp_key_words")


def run(a):
    import bench
    from kelpie_amd import NecessaryPostTrainingEngine
    wl = dict(bench.WORKLOADS[a.workload], _name=a.workload)
    assert wl["mode"] == "necessary", "singleton batches of a necessary workload"
    ds, model, _ = bench.build(wl, 0, 0)
    per_step = wl.get("preds_per_step", 1)
    preds = bench.pick_preds(ds, (a.steps + 1) * per_step, seed=1234)
    jobs = [[(p, [[c] for c in bench.candidates_of(ds, p, wl["candidates"])])
             for p in preds[i * per_step:(i + 1) * per_step]] for i in range(a.steps + 1)]
    ctx = model.ctx
    sent = {"bytes": 0}
    orig = ctx.posttrain_rank

    def counted(hp, x0, row_off, rows, rng_off, rng, *rest, **kw):
        n = len(row_off) - 1
        sent["bytes"] += 16 * n if x0 is None else x0.nbytes + 4 * int(rng_off[-1]) + rng_off.nbytes
        return orig(hp, x0, row_off, rows, rng_off, rng, *rest, **kw)

    ctx.posttrain_rank = counted
    for pair in range(a.pairs):
        for mode in a.modes.split(","):
            eng = NecessaryPostTrainingEngine(model, ds, wl["hp"])
            eng.draws, eng.seed = mode, 42
            bench.seed_all(42)
            acc = {"schedule_s": 0.0, "pack_s": 0.0, "lib_s": 0.0, "device_s": 0.0}
            n = slots = 0
            for i, items in enumerate(jobs):
                eng.set_cache()
                if i == 1:  # the first batch warms the context up
                    sent["bytes"], t0 = 0, time.perf_counter()
                out = eng.compute_relevance_multi(items)
                if i >= 1:
                    n += sum(len(o) for o in out)
                    slots += eng.last_batch_stats.get("slots") or 0
                    for k in acc:
                        acc[k] += float(eng.last_batch_stats.get(k) or 0.0)
            wall = time.perf_counter() - t0
            print(json.dumps({"workload": a.workload, "draws": mode, "pair": pair, "batches": a.steps, "candidates": n,
                              "slots": slots, "cand_per_s": round(n / wall, 1),
                              "ms_per_batch": {k[:-2]: round(1e3 * v / a.steps, 3) for k, v in acc.items()},
                              "wall_ms_per_batch": round(1e3 * wall / a.steps, 3),
                              "draw_bytes_per_batch": sent["bytes"] // a.steps}), flush=True)


def summarise(a):
    for db in a.db:
        rows = sqlite3.connect(db).execute("select name, start, end from kernels").fetchall()
        total = sum(e - s for _, s, e in rows)
        per = {k: (sum(e - s for n, s, e in rows if k in n), sum(1 for n, _, _ in rows if k in n)) for k in KEYED}
        print(json.dumps({"db": db, "kernels": len(rows), "device_us": round(total / 1e3, 1),
                          "keyed_us": {k: round(v / 1e3, 1) for k, (v, _) in per.items()},
                          "keyed_launches": {k: c for k, (_, c) in per.items()},
                          "keyed_share": round(sum(v for v, _ in per.values()) / max(total, 1), 5)}))


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--workload", default="transe-fb15k237-necessary")
    r.add_argument("--pairs", type=int, default=3)
    r.add_argument("--steps", type=int, default=6)
    r.add_argument("--modes", default="reference,keyed")
    s = sub.add_parser("sum")
    s.add_argument("db", nargs="+")
    a = ap.parse_args()
    (run if a.cmd == "run" else summarise)(a)


if __name__ == "__main__":
    main()
