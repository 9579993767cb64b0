"""The temporal filter after its two changes — the three `/ 65535.0f` per tap taken through the fp64 reciprocal, and the
tiled kernel's window loop software-pipelined (frame t + 1 loaded while frame t's taps run) — against the oracle's
`temporal_filter`, bit for bit, for both kernels (`k_temporal_tiled`, and `k_temporal` through DERP_NO_TEMPORAL_TILE):
clamped windows (the first and last frames of a sequence), masked pixels, windows longer than one launch's 31 frames (the
carry path), sizes that are no multiple of the 32 x 8 block, and radii 0-4, 16 and 17 (radius 3: a tile of more than
512 cells, whose tail is loaded outside the pipeline; 16 and 17: the last radius whose tile fits in LDS and the first
that does not). With DERP_PARENT_LIB naming an earlier build of
the library, the same inputs go through it in a child process and must give the same bits too."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = (0.01, 0.5, 1.0, 0.5)  # sigma, weights b g r as the sequence driver passes them


def test_division_by_65535_through_the_reciprocal_is_exact():
    """Every colour difference the kernels can meet: RN32(RN64(d * RN64(1 / 65535))) == RN32(d / 65535)."""
    d = np.arange(-65535, 65536, dtype=np.int32)
    want = d.astype(np.float32) / np.float32(65535.0)
    got = (d.astype(np.float64) * (1.0 / 65535.0)).astype(np.float32)
    assert want.dtype == np.float32 and np.array_equal(want.view(np.uint32), got.view(np.uint32))


def _inputs(seed, w, h, n, hole_rows=False):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([(xx * 257 + yy * 131) % 65536, (xx * 97 + yy * 389 + 9000) % 65536, (xx * 31 + yy * 53) % 65536],
                    axis=-1).astype(np.int64)
    guides = [np.clip(base + rng.integers(-300, 300, size=base.shape), 0, 65535).astype(np.uint16) for _ in range(n)]
    disps = [(1.0 / rng.uniform(0.6, 30.0, size=(h, w))).astype(np.float32) for _ in range(n)]
    masks = [(rng.random((h, w)) > 0.15).astype(np.uint8) for _ in range(n)]
    if hole_rows:
        for m in masks[::2]:
            m[h // 3:h // 3 + 4] = 0
    return guides, disps, masks


def _differ(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return int((~((a == b) | (np.isnan(a) & np.isnan(b)))).sum())


CASES = [  # seed, w, h, frames, radius, offsets of the filtered frame in the window
    (1, 75, 37, 5, 1, (0, 2, 4)),
    (2, 64, 16, 3, 2, (0, 1, 2)),
    (3, 45, 29, 4, 3, (0, 3)),
    (4, 33, 9, 35, 1, (0, 17, 34)),  # two launches: the sums travel through the carry buffer
    (5, 5, 3, 3, 2, (1,)),  # smaller than the halo: every tap clamps
    (6, 33, 9, 2, 0, (0, 1)),  # radius 0: one tap per frame, a tile without a halo
    (7, 70, 20, 3, 4, (0, 2)),
    (8, 33, 9, 3, 16, (0, 2)),  # the largest radius the tiled kernel takes: 2560 cells, ten passes of its tail loader
    (9, 33, 9, 3, 17, (0, 2)),  # the smallest one that goes to the direct kernel either way
    (10, 5, 3, 2, 16, (0, 1)),  # the same two radii on an image far smaller than the halo
    (11, 5, 3, 2, 17, (0, 1)),
]


def takes_tiled_kernel(radius):
    """The host's choice restated (temporal_launch in csrc/derp_capi.hip): two LDS buffers of (32 + 2r) x (8 + 2r) cells
    of 9 bytes, each rounded up to 16, must fit 48 KiB. The context does not report which kernel ran, so the formula is
    what pins that the cases above sit on either side of the switch."""
    return radius >= 0 and 2 * (((32 + 2 * radius) * (8 + 2 * radius) * 9 + 15) & ~15) <= 48 * 1024


def test_cases_sit_on_both_sides_of_the_tiled_kernels_limit():
    assert takes_tiled_kernel(16) and not takes_tiled_kernel(17)
    assert 2 * (((32 + 32) * (8 + 32) * 9 + 15) & ~15) == 46080
    radii = {c[4] for c in CASES}
    assert {0, 16, 17} <= radii and all(takes_tiled_kernel(r) for r in radii if r <= 16)


def _gpu(monkeypatch, direct):
    from facebook360_dep_amd import derp, synth

    if direct:
        monkeypatch.setenv("DERP_NO_TEMPORAL_TILE", "1")
    else:
        monkeypatch.delenv("DERP_NO_TEMPORAL_TILE", raising=False)
    n, res, _ = synth.config("tiny")
    return derp.Derp(synth.make_rig(n, res)["cameras"], partial_coverage=1)


@pytest.mark.gpu
@pytest.mark.parametrize("direct", [False, True], ids=["tiled", "direct"])
def test_temporal_kernels_match_the_oracle_bit_for_bit(built, monkeypatch, direct):
    from oracle import oracle_lib as O

    g = _gpu(monkeypatch, direct)
    try:
        for seed, w, h, n, radius, offsets in CASES:
            guides, disps, masks = _inputs(seed, w, h, n, hole_rows=True)
            for off in offsets:
                want = O.temporal_filter(guides, disps, masks, off, ARGS[0], radius, *ARGS[1:])
                got = g.temporal_filter(guides, disps, masks, off, ARGS[0], radius, *ARGS[1:])
                print("temporal %s seed %d %dx%d n %d r %d off %d: %d differ" %
                      ("direct" if direct else "tiled", seed, w, h, n, radius, off, _differ(got, want)))
                assert _differ(got, want) == 0, (seed, w, h, n, radius, off)
            # a window clamped at the sequence's start and end: the first / last frames filtered over a shorter window
            for lo, hi, off in ((0, min(2, n - 1), 0), (max(n - 3, 0), n - 1, n - 1 - max(n - 3, 0))):
                sub = [x[lo:hi + 1] for x in (guides, disps, masks)]
                want = O.temporal_filter(*sub, off, ARGS[0], radius, *ARGS[1:])
                got = g.temporal_filter(*sub, off, ARGS[0], radius, *ARGS[1:])
                assert _differ(got, want) == 0, ("clamped", seed, lo, hi, off)
    finally:
        g.close()


_CHILD = """
import sys, numpy as np
sys.path.insert(0, %r)
from tests import test_gpu_temporal_pipeline as T
from facebook360_dep_amd import derp, synth
n, res, _ = synth.config("tiny")
g = derp.Derp(synth.make_rig(n, res)["cameras"], partial_coverage=1)
out = {}
for seed, w, h, n, radius, offsets in T.CASES:
    guides, disps, masks = T._inputs(seed, w, h, n, hole_rows=True)
    for off in offsets:
        out["%%d_%%d" %% (seed, off)] = g.temporal_filter(guides, disps, masks, off, T.ARGS[0], radius, *T.ARGS[1:])
g.close()
np.savez(sys.argv[1], **out)
"""


@pytest.mark.gpu
@pytest.mark.parametrize("direct", [False, True], ids=["tiled", "direct"])
def test_temporal_kernels_match_an_earlier_build(built, monkeypatch, tmp_path, direct):
    """Only with DERP_PARENT_LIB set (a developer's A/B): the library of the commit before, same inputs, same bits."""
    parent = os.environ.get("DERP_PARENT_LIB")
    if not parent:
        pytest.skip("DERP_PARENT_LIB not set: no earlier build to compare with")
    env = dict(os.environ, DERP_LIB=parent)
    env.pop("DERP_NO_TEMPORAL_TILE", None)
    if direct:
        env["DERP_NO_TEMPORAL_TILE"] = "1"
    path = str(tmp_path / "parent.npz")
    subprocess.run([sys.executable, "-c", _CHILD % ROOT, path], check=True, env=env, timeout=600)
    old = np.load(path)
    g = _gpu(monkeypatch, direct)
    try:
        for seed, w, h, n, radius, offsets in CASES:
            guides, disps, masks = _inputs(seed, w, h, n, hole_rows=True)
            for off in offsets:
                got = g.temporal_filter(guides, disps, masks, off, ARGS[0], radius, *ARGS[1:])
                assert _differ(got, old["%d_%d" % (seed, off)]) == 0, (seed, off)
    finally:
        g.close()
