"""The table budget -> the destination batch of a level (plan_table_batch, through derp_host_table_batch): how many
destinations' projection tables fit the budget, stored inverse warps as soon as the level runs in batches, equal-sized
batches. Pure host arithmetic; the expected values come from the rule as restated here."""
import pytest

PAIRS = [(1000, 1300), (7, 9), (123457, 123457 + 65536)]  # bytes per destination (no inverse warps, with them)


def _rule(D, per_no, per_inv, needed, budget):
    """-> (DB, store_inverse, DB before the batches are equalised), or None when not even one destination fits"""
    inv = bool(needed)
    db = min(D, budget // (per_inv if inv else per_no))
    if db < D and not inv:
        inv = True
        db = min(D, budget // per_inv)
    if db < 1:
        return None
    batches = -(-D // db)
    return -(-D // batches), inv, db


def _budgets(D, per_no, per_inv):
    """from just below one destination to above D destinations, with the boundaries k * per and k * per - 1 of both sizes"""
    out = {0, per_no - 1, (D + 1) * per_inv, D * per_inv + per_inv // 2}
    for per in (per_no, per_inv):
        for k in range(1, D + 2):
            out |= {k * per - 1, k * per, k * per + 1}
    return sorted(out)


def test_sweep(built):
    from facebook360_dep_amd import derp

    checked = refused = 0
    for D in range(1, 65):
        for per_no, per_inv in PAIRS:
            for needed in (False, True):
                for budget in _budgets(D, per_no, per_inv):
                    want = _rule(D, per_no, per_inv, needed, budget)
                    if want is None:
                        with pytest.raises(ValueError):
                            derp.host_table_batch(D, per_no, per_inv, needed, budget)
                        refused += 1
                        continue
                    db, inv = derp.host_table_batch(D, per_no, per_inv, needed, budget)
                    where = (D, per_no, per_inv, needed, budget)
                    assert (db, inv) == want[:2], where
                    assert 1 <= db <= D, where
                    assert db * (per_inv if inv else per_no) <= budget, where
                    batches = -(-D // want[2])
                    assert -(-D // db) == batches, where  # equalising keeps the batch count ...
                    assert db == -(-D // batches), where  # ... and makes the batches as equal as they get
                    assert inv == (needed or db < D), where
                    checked += 1
    assert checked > 20000 and refused > 500


def test_named_cases(built):
    from facebook360_dep_amd import derp

    per_no, per_inv = PAIRS[0]
    # 24 destinations under a 23-destination budget run as 12 + 12, not 23 + 1
    assert derp.host_table_batch(24, per_no, per_inv, True, 23 * per_inv) == (12, True)
    assert derp.host_table_batch(24, per_no, per_inv, False, 24 * per_no - 1) == (12, True)  # (18 fit with inverse warps)
    # everything fits: one batch, inverse warps only if they were needed anyway
    for D in (1, 5, 24, 64):
        for needed in (False, True):
            for budget in (D * per_inv, D * per_inv + 1, 10 * D * per_inv):
                assert derp.host_table_batch(D, per_no, per_inv, needed, budget) == (D, needed)
        assert derp.host_table_batch(D, per_no, per_inv, False, D * per_no) == (D, False)
    # a budget that holds D destinations without inverse warps and only k = 7 < D with them: whole while no inverse
    # warps are stored; two batches of 5 where they are needed anyway, and one byte lower, where batching forces them
    D = 10
    budget = D * per_no
    assert budget // per_inv == (budget - 1) // per_inv == 7
    assert derp.host_table_batch(D, per_no, per_inv, False, budget) == (D, False)
    assert derp.host_table_batch(D, per_no, per_inv, True, budget) == (5, True)
    assert derp.host_table_batch(D, per_no, per_inv, False, budget - 1) == (5, True)
    # one destination fits without inverse warps, but a batch needs them and then none does
    assert derp.host_table_batch(1, per_no, per_inv, False, per_no) == (1, False)
    with pytest.raises(ValueError):
        derp.host_table_batch(2, per_no, per_inv, False, per_inv - 1)


def test_refused(built):
    from facebook360_dep_amd import derp

    per_no, per_inv = PAIRS[0]
    for D in (1, 3, 24):
        for needed, budget in ((True, per_inv - 1), (True, 0), (False, per_no - 1), (False, 0)):
            with pytest.raises(ValueError):
                derp.host_table_batch(D, per_no, per_inv, needed, budget)
    for args in ((0, per_no, per_inv, False, 10 ** 9), (-3, per_no, per_inv, True, 10 ** 9), (4, 0, per_inv, False, 10 ** 9),
                 (4, per_no, 0, True, 10 ** 9), (4, 0, 0, False, 10 ** 9)):
        with pytest.raises(ValueError):
            derp.host_table_batch(*args)
