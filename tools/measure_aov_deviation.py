#!/usr/bin/env python3
"""Record how far float32 arithmetic moves the AOV sample records from their float64 values (CPU only: the oracle,
tests/shading_model.py and tests/aov_model.py).

For every case of aov_model.CASES at the size and sample count of the GPU test: records_f64 (the float64 model over the
oracle's rays, hit lists and random words) against records_f32 (the same features in numpy float32, written from SURVEY 8
a8 / a9), per field in the metric of aov_model.deviation, over the samples that have a surface and are not fragile.  The
largest figure per field goes to tests/golden/aov_tolerance.json; tests/test_aov_gpu.py holds the kernels to twice that
figure, and tests/test_aov_model.py to the condition that at most 1 % of a case's samples are fragile.

    python tools/measure_aov_deviation.py
"""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import __graft_entry__ as entry  # noqa: E402
import aov_model as am  # noqa: E402


def measure(pta, oracle):
    per_case, fields = {}, {k: 0.0 for k in am.FIELDS}
    for name in am.CASES:
        model, scene, camera = am.model_of(name, pta, oracle)
        prof = am.sample_profile(pta)
        rec = am.records_f64(model, prof)
        dev = am.deviation(am.records_f32(model, rec), rec, am.origin_of(camera))
        use = (rec.prim >= 0) & ~rec.fragile
        row = {k: float(v[use].max()) if use.any() else 0.0 for k, v in dev.items()}
        per_case[name] = dict(row, samples=int(rec.prim.size), covered=int((rec.prim >= 0).sum()), fragile=int(rec.fragile.sum()))
        for k, v in row.items():
            fields[k] = max(fields[k], v)
        print(name, per_case[name], file=sys.stderr)
    return {"width": am.SAMPLE_SIZE[0], "height": am.SAMPLE_SIZE[1], "samples": am.SAMPLES, "fields": fields, "cases": per_case}


def main():
    out = measure(entry.load_package(), entry.load_oracle())
    path = ROOT / "tests" / "golden" / "aov_tolerance.json"
    path.write_text(json.dumps(out, indent=1, sort_keys=True) + "\n")
    print("wrote", path, file=sys.stderr)


if __name__ == "__main__":
    main()
