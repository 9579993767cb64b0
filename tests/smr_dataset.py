"""A small SimpleMeshRenderer input tree: rig JSON, color/<cam>/<frame>.png (16-bit BGR) and
disparity/<cam>/<frame>.pfm of a synth rig, the layout the reference's exports stage reads."""
import json
import os


def write(root, n=4, res=48, frames=(0, 1)):
    from facebook360_dep_amd import imageio, synth

    rig = synth.make_rig(n, res)
    os.makedirs(root, exist_ok=True)
    with open(os.path.join(root, "rig.json"), "w") as f:
        json.dump(rig, f)
    data = {}
    for fi in frames:
        fr = synth.make_frame(rig, [(res, res)], frame=fi, device="cpu")
        name = "%06d" % fi
        for ci, cam in enumerate(rig["cameras"]):
            for kind in ("color", "disparity"):
                os.makedirs(os.path.join(root, kind, cam["id"]), exist_ok=True)
            imageio.write_png16(os.path.join(root, "color", cam["id"], name + ".png"), fr["color"][0][ci])
            imageio.write_pfm(os.path.join(root, "disparity", cam["id"], name + ".pfm"), fr["truth"][ci])
        data[fi] = fr
    return rig, data
