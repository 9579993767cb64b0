"""Authoring-time generator (needs the reference tree; never runs on the GPU box or in the test suite).

ref_flags_preview.json: name / type / default / description of every gflags DEFINE_* of the reference's tuning previews
(source/render/ViewColorVarianceThresholds.cpp, source/render/ViewForegroundMaskThresholds.cpp,
source/render/GenerateKeypointProjections.cpp), extracted with the reference's own `get_flags` scraper
(scripts/util/system_util.py:123-176) exactly as gen_ref_pins_sweep.py does. GenerateKeypointProjections also reads flags
the calibration library defines: those it uses are pinned from source/calibration/Calibration.cpp and FeatureMatcher.cpp.

Usage: python tests/golden/gen_ref_pins_preview.py   (from the repo root)
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_ref_pins  # noqa: E402

BINARIES = {
    "ViewColorVarianceThresholds": "source/render/ViewColorVarianceThresholds.cpp",
    "ViewForegroundMaskThresholds": "source/render/ViewForegroundMaskThresholds.cpp",
    "GenerateKeypointProjections": "source/render/GenerateKeypointProjections.cpp",
}
# the calibration library's flags GenerateKeypointProjections reads (the rest of the library's flags are not offered)
LIBRARY = {
    "source/calibration/Calibration.cpp": ["color", "frame", "threads"],
    "source/calibration/FeatureMatcher.cpp": ["depth_max", "depth_min", "depth_samples", "search_overlap", "search_radius"],
}

if __name__ == "__main__":
    get_flags = gen_ref_pins.load_get_flags()
    out = {name: {"source": rel, "flags": get_flags(os.path.join(gen_ref_pins.REF, rel))} for name, rel in BINARIES.items()}
    for rel, names in LIBRARY.items():
        found = {fl["name"]: fl for fl in get_flags(os.path.join(gen_ref_pins.REF, rel))}
        out["GenerateKeypointProjections"]["flags"] += [found[name] for name in names]
    with open(os.path.join(gen_ref_pins.HERE, "ref_flags_preview.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
