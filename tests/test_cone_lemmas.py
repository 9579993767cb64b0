"""The two lemmas behind the cost kernels' FOV-cone test (`sees<LEAN>`, csrc/derp_camera.h), checked in numpy's IEEE
float64 against the reference's expression: dot <= 0 implies outside, dot > kappa |v|_1 implies inside. The device
evaluates the reference's expression itself for everything in between, so these two implications are all that its
exactness rests on (tests/test_gpu_cost_trims.py compares the device with the oracle on the same points)."""
import math

import numpy as np
import pytest

from tests import cone_cases as CC

COS = [math.cos(math.pi / 2), 2.0 ** -100, 1e-9, 0.3, 0.9, 0.999]


@pytest.mark.parametrize("c", COS)
def test_reject_and_accept_agree_with_the_reference(c):
    rng = np.random.default_rng(18)
    st = dict(R=np.eye(3), position=np.zeros(3))
    pts = np.concatenate([CC.camera_space_points(c, rng, per=20000),
                          # the domain's ends: |v|_1 at 2^-400 and just under 2^500
                          CC.camera_space_points(c, rng, per=2000) * 2.0 ** -396 / 0.05,
                          CC.camera_space_points(c, rng, per=2000) * 2.0 ** 460])
    dot, v = CC.computed_dot(st, pts)
    l1 = np.abs(v).sum(1)
    assert l1.min() >= 2.0 ** -400 and l1.max() < 2.0 ** 500
    kind = CC.classify(c, dot, v)
    outside = CC.reference_outside(c, dot, v)
    counts = [int((kind == k).sum()) for k in (CC.REJECT, CC.ACCEPT, CC.FALL_THROUGH)]
    print("cos_fov %.3g: reject / accept / fall-through %s; outside among the fall-through %d" % (
        c, counts, int(outside[kind == CC.FALL_THROUGH].sum())))
    assert min(counts) > 0
    assert outside[kind == CC.REJECT].all()
    assert not outside[kind == CC.ACCEPT].any()
    # the fall-through holds points of both answers, or the sliver would not need the reference's expression
    ft = outside[kind == CC.FALL_THROUGH]
    assert ft.any() and not ft.all()


def test_accept_threshold_is_tight_to_the_margin():
    """the accept threshold sits 2^-20 (relative) outside the cone on the axes, where |v|_1 = |v|_2: nearer, and the
    lemma's roundings would need counting again"""
    c = 0.3
    v = np.array([[0.0, 0.0, -1.0]])
    dot = np.array([c * (1 + 2.0 ** -19)])
    assert CC.classify(c, dot * 3.0, v * 3.0)[0] == CC.ACCEPT
    assert CC.classify(c, np.array([c * 3.0]), v * 3.0)[0] == CC.FALL_THROUGH
