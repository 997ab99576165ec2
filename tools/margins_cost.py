"""What the rank margins cost, and what they say about the full-size fixtures (ANALYSIS TOOL,
DESIGN.md section 6).

    python tools/margins_cost.py run [--workload complex-fb15k237-sufficient] [--rounds 3] [--tol 1e-4]
    rocprofv3 --kernel-trace -d OUT -o run -- python tools/margins_cost.py run ...
    python tools/margins_cost.py sum OUT/.../run_results.db
    python tools/margins_cost.py table [--tol 1e-4] [fixture-name ...]

``run`` evaluates the workload's first singleton batch (bench.py's first prediction) on one
context, without and with ``engine.margin_tol`` alternating, ``--rounds`` counted rounds after
one warm-up round, and prints per round the device time of each call (the context's own
events) and whether the relevances are the same.  ``sum`` splits a kernel trace of such a run
into the rank stage every batch runs and the margin kernels only the batches with margins run.
``table`` replays the ComplEx full-size fixtures (tests/golden/fullsize/complex-*.json) with
margins and counts the rank deltas whose band [post.rank_lo - base.rank_hi, post.rank_hi -
base.rank_lo] is wider than one place.
"""
import argparse
import glob
import json
import os
import sqlite3
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RANK = ("kp_rank_filter_bits", "kp_rank_f64_kelpie", "kp_rank_f64_count", "rankq64")
MARGIN = ("kp_rank_margin_thr", "kp_rank_f64_margin", "kp_rank_margin_merge")


def run(a):
    import bench
    from kelpie_amd import NecessaryPostTrainingEngine, SufficientPostTrainingEngine
    wl = dict(bench.WORKLOADS[a.workload], _name=a.workload)
    ds, model, _ = bench.build(wl, 0, 0)
    suff = wl["mode"] == "sufficient"
    eng = (SufficientPostTrainingEngine if suff else NecessaryPostTrainingEngine)(model, ds, wl["hp"])
    pred = bench.pick_preds(ds, 1, seed=1234)[0]
    cands = [[c] for c in bench.candidates_of(ds, pred, wl["candidates"])]
    item = (pred, cands, eng.select_entities_to_convert(pred, wl["convert"], 200)) if suff else (pred, cands)
    first = None
    for rnd in range(a.rounds + 1):  # round 0 warms the context up
        rec = {"round": rnd, "counted": rnd > 0}
        for tol in (None, a.tol):
            eng.margin_tol = tol
            bench.seed_all(42)
            eng.set_cache()
            out = eng.compute_relevance_multi([item])
            st = eng.last_batch_stats
            key = "with" if tol is not None else "without"
            rec[key + "_device_ms"] = round(1e3 * float(st.get("device_s") or 0.0), 4)
            rec[key + "_lib_ms"] = round(1e3 * float(st.get("lib_s") or 0.0), 4)
            rec["slots"] = st.get("slots")
            first = out if first is None else first
            rec[key + "_same_relevances"] = out == first
        print(json.dumps(rec), flush=True)


def summarise(a):
    for db in a.db:
        rows = sqlite3.connect(db).execute("select name, start, end from kernels").fetchall()
        total = sum(e - s for _, s, e in rows)

        def group(keys):
            return {k: sum(e - s for n, s, e in rows if k in n) for k in keys}

        rank, mg = group(RANK), group(MARGIN)
        batches = max(1, sum(1 for n, _, _ in rows if "kp_rank_f64_kelpie" in n))
        with_mg = max(1, sum(1 for n, _, _ in rows if "kp_rank_margin_merge" in n))
        print(json.dumps({"db": db, "batches": batches, "batches_with_margins": with_mg,
                          "device_us_per_batch_all_kernels": round(total / batches / 1e3, 1),
                          "rank_stage_us_per_batch": round(sum(rank.values()) / batches / 1e3, 1),
                          "rank_us_per_batch": {k: round(v / batches / 1e3, 1) for k, v in rank.items()},
                          "margin_us_per_batch_with_margins": {k: round(v / with_mg / 1e3, 1) for k, v in mg.items()},
                          "margin_stage_us_per_batch_with_margins": round(sum(mg.values()) / with_mg / 1e3, 1)}))


def table(a):
    import bench
    from kelpie_amd import NecessaryPostTrainingEngine, SufficientPostTrainingEngine
    names = a.fixture or sorted(os.path.basename(p)[:-5]
                                for p in glob.glob(os.path.join(ROOT, "tests", "golden", "fullsize", "complex-*.json")))
    built, total = {}, {"fixtures": 0, "elements": 0, "band_of_one_place_or_more": 0, "band_wider_than_one_place": 0}
    for name in names:
        with open(os.path.join(ROOT, "tests", "golden", "fullsize", name + ".json")) as f:
            fx = json.load(f)
        wl = bench.WORKLOADS[fx["workload"]]
        if fx["workload"] not in built:
            built.clear()  # one model resident at a time
            built[fx["workload"]] = bench.build(wl, 0, 0)
        ds, model, _ = built[fx["workload"]]
        suff = wl["mode"] == "sufficient"
        eng = (SufficientPostTrainingEngine if suff else NecessaryPostTrainingEngine)(model, ds, wl["hp"])
        eng.margin_tol = a.tol
        _, _, _, par = bench.parity_sample(eng, wl, fx, None)
        pairs = [pb for rj in eng.last_results for pb in rj] if suff else list(eng.last_results)
        bands = [(pt["margins"]["rank_lo"] - b["margins"]["rank_hi"], pt["margins"]["rank_hi"] - b["margins"]["rank_lo"])
                 for pt, b in pairs]
        width = [hi - lo for lo, hi in bands]
        f64 = fx["runs"]["fp64"]["rank_deltas"]
        differs = [i for i, (g, r) in enumerate(zip(par["gpu_rank_deltas"], f64)) if g != r]
        rec = {"fixture": name, "tol": a.tol, "elements": len(bands), "band_of_one_place_or_more": sum(w >= 1 for w in width),
               "band_wider_than_one_place": sum(w > 1 for w in width), "widest": max(width),
               "differs_from_fp64": differs, "bands_of_those": [bands[i] for i in differs],
               "fp64_inside_band": [bands[i][0] <= f64[i] <= bands[i][1] for i in differs],
               "ties": sum(pt["margins"]["ties"] + b["margins"]["ties"] for pt, b in pairs),
               # the nearest competitor of any post-training behind the fixture's rank deltas, in score units
               "smallest_gap": min(min(m["margins"]["gap_better"], m["margins"]["gap_worse"]) for pb in pairs for m in pb),
               "largest_abs_score": max(abs(m["target_score"]) for pb in pairs for m in pb)}
        if name == "complex-fb15k237-necessary__p0":
            rec["element_9"] = {"gpu": par["gpu_rank_deltas"][9], "fp64": f64[9], "band": bands[9],
                                "post": pairs[9][0]["margins"], "base": pairs[9][1]["margins"]}
        print(json.dumps(rec), flush=True)
        total["fixtures"] += 1
        for k in ("elements", "band_of_one_place_or_more", "band_wider_than_one_place"):
            total[k] += rec[k]
    print(json.dumps(total), flush=True)


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--workload", default="complex-fb15k237-sufficient")
    r.add_argument("--rounds", type=int, default=3)
    r.add_argument("--tol", type=float, default=1e-4)
    s = sub.add_parser("sum")
    s.add_argument("db", nargs="+")
    t = sub.add_parser("table")
    t.add_argument("--tol", type=float, default=1e-4)
    t.add_argument("fixture", nargs="*")
    a = ap.parse_args()
    {"run": run, "sum": summarise, "table": table}[a.cmd](a)


if __name__ == "__main__":
    main()
