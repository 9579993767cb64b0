"""Authoring-time generator (needs the reference tree; never runs on the GPU box or in the test suite).

ref_flags_align_colors.json: name / type / default / description of every gflags DEFINE_* of the reference's AlignColors
(source/calibration/AlignColors.cpp), extracted with the reference's own `get_flags` scraper
(scripts/util/system_util.py:123-176) exactly as gen_ref_pins_sweep.py does.

Usage: python tests/golden/gen_ref_pins_align_colors.py   (from the repo root)
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_ref_pins  # noqa: E402

BINARIES = {
    "AlignColors": "source/calibration/AlignColors.cpp",
}

if __name__ == "__main__":
    get_flags = gen_ref_pins.load_get_flags()
    out = {name: {"source": rel, "flags": get_flags(os.path.join(gen_ref_pins.REF, rel))} for name, rel in BINARIES.items()}
    with open(os.path.join(gen_ref_pins.HERE, "ref_flags_align_colors.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
