"""What ``precision = "fp64"`` costs, and its parity column (ANALYSIS TOOL, DESIGN.md
sections 3 and 6; runs on the GPU, reads the committed fixtures only).

    python tools/f64_cost.py cost [--workload complex-fb15k237-sufficient] [--rounds 3]
    python tools/f64_cost.py table [fixture-name ...]

``cost``: one singleton batch of the workload (bench.py's first prediction, its candidates and
conversion entities) on one context, the default path and fp64 alternating on the same box:
device ms per batch and per optimizer step (kp_last_timing: one attention launch per step),
the attention's time and its share of the fp64 MFMA peak -- 4 D flops per (query, entity)
pair for S and O together, against AMD's published 78.6 TFLOPS fp64 matrix peak of the
MI355X.  The first batch of either precision warms the context and is not counted.

``table``: for every ComplEx full-size fixture (tests/golden/fullsize), the rank deltas of the
default path and of fp64 that equal the reference's fp64 run's, element by element.
"""
import argparse
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F64_MFMA_PEAK = 78.6e12


def _engine(wl):
    import bench
    from kelpie_amd import NecessaryPostTrainingEngine, SufficientPostTrainingEngine
    ds, model, _ = bench.build(wl, 0, 0)
    cls = SufficientPostTrainingEngine if wl["mode"] == "sufficient" else NecessaryPostTrainingEngine
    return ds, model, cls(model, ds, wl["hp"])


def cost(a):
    import bench
    wl = bench.WORKLOADS[a.workload]
    ds, model, eng = _engine(wl)
    pred = bench.pick_preds(ds, 1, seed=1234)[0]
    cands = [[c] for c in bench.candidates_of(ds, pred, wl["candidates"])]
    if wl["mode"] == "sufficient":
        bench.seed_all(42)
        eng.entities_to_convert = eng.select_entities_to_convert(pred, wl["convert"], 200)
    dp = model.ctx.dim if model.ctx.dim % 16 == 0 else (model.ctx.dim + 15) // 16 * 16
    runs = {"fp32": [], "fp64": []}
    for i in range(a.rounds + 1):
        for prec in ("fp32", "fp64"):
            eng.precision = prec
            eng.set_cache()
            bench.seed_all(42)
            eng.compute_relevance_batch(pred, cands)
            st = eng.last_batch_stats
            if i:  # the first round warms both paths
                runs[prec].append((st["device_s"], st["hot_s"], st["hot_launches"], st["slots"],
                                   model.ctx.last_timing().get("hot_work", 0.0)))
    out = {"workload": a.workload, "rounds": a.rounds, "row_width": dp}
    for prec, rs in runs.items():
        dev = sorted(r[0] for r in rs)[len(rs) // 2]
        hot = sorted(r[1] for r in rs)[len(rs) // 2]
        steps, slots, work = rs[0][2], rs[0][3], rs[0][4]
        out[prec] = {"slots": slots, "steps": steps, "device_ms": round(dev * 1e3, 3),
                     "ms_per_step": round(dev * 1e3 / max(1, steps), 4), "attention_ms": round(hot * 1e3, 3),
                     "device_ms_all": [round(r[0] * 1e3, 3) for r in rs]}
        if prec == "fp64" and hot > 0:
            flops = 4.0 * dp * work
            out[prec]["attention_tflops"] = round(flops / hot / 1e12, 3)
            out[prec]["attention_share_of_f64_mfma_peak"] = round(flops / hot / F64_MFMA_PEAK, 4)
    out["fp64_over_fp32"] = round(out["fp64"]["device_ms"] / out["fp32"]["device_ms"], 2)
    print(json.dumps(out), flush=True)


def table(a):
    import bench
    fdir = os.path.join(ROOT, "tests", "golden", "fullsize")
    names = a.fixtures or sorted(os.path.basename(p)[:-5] for p in glob.glob(os.path.join(fdir, "complex-*.json")))
    built, tot = {}, {"elements": 0, "fp32_equal": 0, "fp64_equal": 0}
    for name in names:
        with open(os.path.join(fdir, name + ".json")) as f:
            fx = json.load(f)
        wl = bench.WORKLOADS[fx["workload"]]
        if fx["workload"] not in built:
            built.clear()  # one model resident at a time
            built[fx["workload"]] = _engine(wl)
        _, _, eng = built[fx["workload"]]
        ref = fx["runs"]["fp64"]["rank_deltas"]
        row = {"fixture": name, "elements": len(ref)}
        for prec in ("fp32", "fp64"):
            eng.precision = prec
            _, _, _, par = bench.parity_sample(eng, wl, fx, None)
            row[prec + "_equal"] = sum(x == y for x, y in zip(par["gpu_rank_deltas"], ref))
            row[prec + "_device_ms"] = round(eng.last_batch_stats["device_s"] * 1e3, 1)
        row["ref_fp32_equal"] = sum(x == y for x, y in zip(fx["runs"]["fp32"]["rank_deltas"], ref))
        for k in tot:
            tot[k] += row[k]
        print(json.dumps(row), flush=True)
    print(json.dumps({"total": tot}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    c = sub.add_parser("cost")
    c.add_argument("--workload", default="complex-fb15k237-sufficient")
    c.add_argument("--rounds", type=int, default=3)
    t = sub.add_parser("table")
    t.add_argument("fixtures", nargs="*")
    a = ap.parse_args()
    (cost if a.cmd == "cost" else table)(a)


if __name__ == "__main__":
    main()
