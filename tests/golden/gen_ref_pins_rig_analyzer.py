"""Authoring-time generator (needs the reference tree; never runs on the GPU box or in the test suite).

ref_flags_rig_analyzer.json: name / type / default / description of every gflags DEFINE_* of the reference's RigAnalyzer
(source/rig/RigAnalyzer.cpp), extracted with the reference's own `get_flags` scraper (scripts/util/system_util.py:123-176)
exactly as gen_ref_pins.py does for ref_flags.json.

Usage: python tests/golden/gen_ref_pins_rig_analyzer.py   (from the repo root)
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_ref_pins  # noqa: E402

BINARIES = {"RigAnalyzer": "source/rig/RigAnalyzer.cpp"}


def trimmed(flags):
    """The scraper ends a description at the next DEFINE_; after the file's last flag it runs on into the code that
    follows. A description is string literals only, so it ends at the `);` that closes its DEFINE_."""
    for f in flags:
        f["descr"] = f["descr"].split(");")[0]
    return flags


if __name__ == "__main__":
    get_flags = gen_ref_pins.load_get_flags()
    out = {name: {"source": rel, "flags": trimmed(get_flags(os.path.join(gen_ref_pins.REF, rel)))} for name, rel in BINARIES.items()}
    with open(os.path.join(gen_ref_pins.HERE, "ref_flags_rig_analyzer.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
