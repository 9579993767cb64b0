"""Named cases of the AlignColors tests: small rigs with their three one-camera reference rigs, each built to contain
one thing that tests/test_align_ref.py asserts it really contains (on the restatement, without a GPU), so that a case
cannot quietly stop exercising its branch. tests/test_gpu_align.py runs every case on the device."""
import numpy as np

from tests import align_ref as R


def camera(cam_id, w, h, focal, principal=None, distortion=None, cam_type="FTHETA", index=0):
    cam = dict(version=1, type=cam_type, id=cam_id, origin=[0.1 * index, 0.0, 0.0], forward=[0.0, 0.0, -1.0],
               up=[0.0, 1.0, 0.0], right=[1.0, 0.0, 0.0], resolution=[w, h], focal=[focal, -focal])
    if principal is not None:
        cam["principal"] = list(principal)
    if distortion is not None:
        cam["distortion"] = list(distortion)
    return cam


def _refs(red, green, blue):
    """the three reference rigs' single cameras: (focal, distortion or None) each, on a 1000 x 1000 sensor"""
    return tuple(camera("ref", 1000, 1000, f, distortion=d) for f, d in (red, green, blue))


def _case(name, rig, refs, cameras=""):
    return dict(name=name, rig=rig, red_ref=refs[0], green_ref=refs[1], blue_ref=refs[2], cameras=cameras)


MILD = ((1006.0, [-0.028, 0.0015]), (1000.0, [-0.03, 0.002]), (995.0, [-0.033, 0.0025, -0.0001]))


def all_cases():
    cases = [
        # a size that is a multiple of no block and no run of pixels; principal off-centre by no half pixel
        _case("odd_37x23", [camera("cam0", 37, 23, 20.0, (17.3, 12.9), [-0.03, 0.002])], _refs(*MILD)),
        # principal exactly on the centre of pixel (8, 5): the n == 0 rule, at exactly one pixel
        _case("principal_on_centre", [camera("cam0", 16, 12, 9.0, (8.5, 5.5), [-0.03, 0.002])], _refs(*MILD)),
        _case("principal_outside", [camera("cam0", 24, 16, 30.0, (-6.25, 20.75), [-0.03, 0.002])], _refs(*MILD)),
        # green without distortion (undistort's short circuit), red and blue with
        _case("zero_green_distortion", [camera("cam0", 30, 20, 14.0, (15.2, 9.7))],
              _refs((1006.0, [-0.028, 0.0015]), (1000.0, None), (995.0, [0.02]))),
        # ... and its mirror: red without, green with
        _case("zero_red_distortion", [camera("cam0", 30, 20, 14.0, (15.2, 9.7), [-0.03, 0.002])],
              _refs((1006.0, None), (1000.0, [-0.03, 0.002]), (995.0, [0.0, 0.0, 0.0]))),
        # distortion negative and strong: distortionMax is finite (green 1.29, red 1.15, blue 1.23 rad), the corners lie
        # beyond distort(distortionMax) of green, and green's angle there exceeds red's and blue's distortionMax
        _case("clamped_rim", [camera("cam0", 48, 32, 20.0, (24.3, 15.8), [-0.2])],
              _refs((1004.0, [-0.25]), (1000.0, [-0.2]), (997.0, [-0.22]))),
        # no distortion anywhere and focal ratios of exactly 2 and 0.5 about a principal point on a pixel centre: red targets
        # leave the image on every side, and every red coordinate is k + 0.5 (round's tie), every other blue one too
        _case("leaves_image", [camera("cam0", 32, 24, 10.0, (16.5, 12.5))], _refs((20.0, None), (10.0, None), (5.0, None))),
        # 1234.567 / 1000 is no float: the reference's float focalRatio is part of the result
        _case("float_ratio", [camera("cam0", 40, 30, 1234.567, (19.7, 15.4), [-0.03, 0.002])], _refs(*MILD)),
        # three cameras of two resolutions and two types, a subset in another order
        _case("mixed_rig", [camera("cam0", 40, 28, 22.0, (20.4, 13.7), [-0.03, 0.002], index=0),
                            camera("cam1", 96, 64, 70.0, (47.1, 32.6), [-0.01], cam_type="RECTILINEAR", index=1),
                            camera("cam2", 40, 28, 21.5, (19.2, 14.9), [-0.035, 0.001], index=2)],
              _refs(*MILD), cameras="cam2,cam1"),
    ]
    return {c["name"]: c for c in cases}


def selected(case):
    """image_util::filterDestinations (ImageUtil.cpp:110-125): the case's rig after --cameras"""
    if not case["cameras"]:
        return list(case["rig"])
    return [cam for name in case["cameras"].split(",") for cam in case["rig"] if cam["id"] == name]


def images(case, frame=0):
    """per selected camera one random BGR u16 image with runs of 0 and of 65535 in it"""
    out = []
    for k, cam in enumerate(selected(case)):
        rng = np.random.default_rng([sum(map(ord, case["name"])), frame, k])
        w, h = cam["resolution"]
        im = rng.integers(0, 65536, size=(h, w, 3), dtype=np.uint16)
        im[rng.random((h, w)) < 0.1] = 0
        im[rng.random((h, w)) < 0.1] = 65535
        out.append(im)
    return out


_EXPECTED = {}


def expected(case, frame=0):
    """the restatement's maps and aligned images of the case: computed once, shared, read-only
    -> list per selected camera of (red map, blue map, aligned image)"""
    key = (case["name"], frame)
    if key not in _EXPECTED:
        out = []
        for cam, im in zip(selected(case), images(case, frame)):
            red, blue = R.maps_of(cam, case["red_ref"], case["green_ref"], case["blue_ref"])
            aligned = R.align(im, red, blue)
            for a in (red, blue, aligned):
                a.setflags(write=False)
            out.append((red, blue, aligned))
        _EXPECTED[key] = out
    return _EXPECTED[key]
