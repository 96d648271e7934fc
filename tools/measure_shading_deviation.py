#!/usr/bin/env python3
"""Measures how far the CPU oracle sits from the float64 shading model (tests/shading_model.py) over the feature matrix
(tests/scene_builder.py) and writes tests/golden/shading_model_deviation.json: per tier (direct; whole paths per depth) the
largest and the 99.9th-percentile relative radiance deviation, the largest ray disagreement, and per case the share of
fragile paths.  tests/test_shading_model.py reads its tolerances from that file.  No GPU.

    python tools/measure_shading_deviation.py [--jobs N] [--only CASE ...] [--no-write]
"""
import argparse
import json
import sys
from concurrent.futures import ProcessPoolExecutor
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
OUT = ROOT / "tests" / "golden" / "shading_model_deviation.json"


def measure(job):
    import shading_model as sm
    name, bounces = job
    frame = sm.Frame(sm.model_job(job))
    results, stats = frame.results, {"numeric_errors": frame.numeric_errors}
    excess, atol, kind_mismatch, fragile = sm.compare(frame.oracle_accum, results)
    keep = ~fragile
    reasons = {}
    for r in results:
        if r.fragile:
            reasons[r.fragile] = reasons.get(r.fragile, 0) + 1
    return dict(case=name, tier=sm.tier_of(bounces), excess=excess[keep].reshape(-1).tolist(),
                ray=max([r.ray_error for r, k in zip(results, keep) if k], default=0.0), fragile=float(fragile.mean()),
                reasons=reasons, kind_mismatch=kind_mismatch, numeric_errors=stats["numeric_errors"],
                alive=float(np.mean([r.alive_at_last for r in results])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--only", nargs="*")
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    import scene_builder as sb
    jobs = []
    for c in sb.cases():
        if args.only and c.name not in args.only:
            continue
        jobs.append((c.name, 0))
        if c.bounces:
            jobs.append((c.name, c.bounces))
    with ProcessPoolExecutor(args.jobs) as pool:
        rows = list(pool.map(measure, jobs))
    tiers, fragile_share, alive = {}, {}, {}
    for r in rows:
        t = tiers.setdefault(r["tier"], dict(excess=[], ray=0.0, cases=0))
        t["excess"] += r["excess"]
        t["ray"] = max(t["ray"], r["ray"])
        t["cases"] += 1
        fragile_share[f'{r["case"]}@{r["tier"]}'] = round(r["fragile"], 5)
        if r["tier"] != "direct":
            alive[r["case"]] = round(r["alive"], 4)
        flag = "" if r["kind_mismatch"] == 0 and r["numeric_errors"] == 0 else "   <-- kind mismatch / numeric errors"
        print(f'{r["case"]:32s} {r["tier"]:7s} max {max(r["excess"], default=0):.3e} ray {r["ray"]:.3e} fragile {r["fragile"]:.4f} '
              f'alive {r["alive"]:.2f} {r["reasons"]}{flag}')
    doc = {"comment": "written by tools/measure_shading_deviation.py: the CPU oracle against tests/shading_model.py",
           "tiers": {}, "fragile_share": fragile_share, "alive_at_last_bounce": alive}
    for name, t in sorted(tiers.items()):
        e = np.array(t["excess"])
        doc["tiers"][name] = {"cases": t["cases"], "values": int(e.size), "max_rel": float(e.max()),
                              "p999_rel": float(np.percentile(e, 99.9)), "max_ray": t["ray"]}
        print(name, doc["tiers"][name])
    if not args.no_write and not args.only:
        OUT.write_text(json.dumps(doc, indent=1, sort_keys=True) + "\n")
        print("wrote", OUT)


if __name__ == "__main__":
    main()
