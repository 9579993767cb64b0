"""Authoring-time generator (needs the reference tree; never runs on the GPU box or in the test suite).

ref_flags_create_obj_from_disparity_equirect.json: name / type / default / description of every gflags DEFINE_* of the
reference's CreateObjFromDisparityEquirect (source/conversion/CreateObjFromDisparityEquirect.cpp:36-45) and PngToPfm
(source/conversion/PngToPfm.cpp:28-29), extracted with the reference's own `get_flags` scraper
(scripts/util/system_util.py:123-176) exactly as gen_ref_pins.py does for ref_flags.json.

Usage: python tests/golden/gen_ref_pins_create_obj_from_disparity_equirect.py   (from the repo root)
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_ref_pins  # noqa: E402

BINARIES = {"CreateObjFromDisparityEquirect": "source/conversion/CreateObjFromDisparityEquirect.cpp",
            "PngToPfm": "source/conversion/PngToPfm.cpp"}

if __name__ == "__main__":
    get_flags = gen_ref_pins.load_get_flags()
    out = {name: {"source": rel, "flags": get_flags(os.path.join(gen_ref_pins.REF, rel))} for name, rel in BINARIES.items()}
    with open(os.path.join(gen_ref_pins.HERE, "ref_flags_create_obj_from_disparity_equirect.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
