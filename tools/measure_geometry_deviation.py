#!/usr/bin/env python3
"""Measures how far the f32 layer of the geometry model (tests/geometry_model.py) sits from its float64 layer on the
well-conditioned pairs of gen_pairs() and writes tests/golden/geometry_model_deviation.json; tests/test_geometry_model.py
asserts a ceiling of twice the recorded values.  No GPU, no oracle.

    python tools/measure_geometry_deviation.py [--no-write]
"""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
OUT = ROOT / "tests" / "golden" / "geometry_model_deviation.json"


def main():
    import geometry_model as gm
    g = gm.guard(*gm.gen_pairs())
    record = {"set": "geometry_model.gen_pairs(): the pairs well_conditioned() keeps (every decision reached in float64 at least "
                     "`margin` from its threshold and further from it than the a-priori f32 rounding bound)",
              "seed": gm.PAIR_SEED, "pairs_generated": gm.PAIR_COUNT, "margin": gm.MARGIN, "pairs": g["pairs"], "hits": g["hits"],
              "verdict_mismatches": g["verdict_mismatches"],
              "deviation": g["deviation"],
              "deviation_is": "largest |f32 - float64|: dist relative to |dist|, u and v absolute, over the accepted pairs of the set"}
    print(json.dumps(record, indent=1))
    if "--no-write" not in sys.argv:
        OUT.write_text(json.dumps(record, indent=1) + "\n")


if __name__ == "__main__":
    main()
