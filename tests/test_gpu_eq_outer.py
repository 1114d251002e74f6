"""GPU tier: eq tables above 2^13 entries, built as the outer product of two half tables (three launches), against the same table
built level by level (COZK_EQ_LEVELS, read on every call) and, at the two smallest sizes, against the oracle."""
import numpy as np
import pytest

import pyref as O

pytestmark = pytest.mark.gpu


# odd and even nv (m = ceil(nv / 2): the halves differ in size for odd nv); 14 is the first size of the new path (m = 7: a wave of
# 64 lanes still shares its hi entry, a workgroup of 256 does not), 20 and 21 span more than one pass of the capped grid
@pytest.mark.parametrize("nv", [14, 15, 20, 21])
def test_eq_evals_outer_product_equals_level_path(cozk, ctx, monkeypatch, nv):
    rng = O.SplitMix64(900 + nv)
    r = [rng.field() for _ in range(nv)]
    monkeypatch.delenv("COZK_EQ_LEVELS", raising=False)
    outer = cozk.eq_evals(ctx, r).to_numpy()
    monkeypatch.setenv("COZK_EQ_LEVELS", "1")
    levels = cozk.eq_evals(ctx, r).to_numpy()
    assert outer.shape == levels.shape == (1 << nv, 4)
    assert np.array_equal(outer, levels)  # the stored bytes: both paths store canonical Montgomery forms
    if nv <= 15:
        assert cozk.mont_limbs_to_int(outer) == O.eq_evals(r)  # r[0] in the most significant index bit
