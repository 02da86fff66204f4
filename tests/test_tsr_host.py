"""Host side of the time-scale regression (CPU only): TimeScaleOLS from a hand-made statistics
array against closed forms, and the operand checks of ops.dwt_time_scale_regression, which
run before the device check (the pattern of tests/test_ops_validation.py)."""

import numpy as np
import pytest
import torch

from wtmi import ops
from wtmi.transforms import TimeScaleOLS

X = torch.zeros(2, 64)
LO = np.ones(8)


def test_time_scale_ols_closed_forms():
    # df_resid = 1: Student t is Cauchy, two-sided p = 1 - 2 atan|t| / pi
    # const, slope, bse_const, bse_slope, rsquared, ssr, nobs, df_resid
    stats = np.array([[1.0, 2.0, 1.0, 0.02, 0.9, 3.0, 3, 1],
                      [-7.0, 0.1, 1.0, 0.1, 0.5, 3.0, 3, 1],
                      [0.0, 30.0, 2.0, 1.0, 0.1, 3.0, 3, 1]])
    r = TimeScaleOLS.from_stats(stats)
    assert r.names == ["S_2", "D_2", "D_1"] and (r.nobs, r.df_resid) == (3, 1)
    t = np.array([[1.0, 100.0], [-7.0, 1.0], [0.0, 30.0]])
    np.testing.assert_allclose(r.tvalues, t, rtol=1e-15)
    np.testing.assert_allclose(r.pvalues, 1 - 2 * np.arctan(np.abs(t)) / np.pi, rtol=1e-12)
    # p = 0.5, 0.0064 | 0.0903, 0.5 | 1, 0.0212
    assert r.stars() == [["", "***"], ["*", ""], ["", "**"]]
    np.testing.assert_array_equal(r.rsquared, [0.9, 0.5, 0.1])
    slope_only = TimeScaleOLS.from_stats(stats, add_constant=False)
    np.testing.assert_array_equal(slope_only.params, stats[:, 1:2])
    assert slope_only.stars() == [["***"], [""], ["**"]]


@pytest.mark.parametrize("x,y,taps,level,msg", [
    (X, torch.zeros(2, 65), (LO, LO, LO, LO), 2, "same shape"),
    (X, torch.zeros(3, 64), (LO, LO, LO, LO), 2, "same shape"),
    (X, X, (LO, LO, LO[:6], LO), 2, "number of taps"),
    (X, X, (LO, LO, LO, LO), -1, "level"),
    (X, X.double(), (LO, LO, LO, LO), 2, "float32"),
])
def test_operand_checks_run_before_the_library(x, y, taps, level, msg, monkeypatch):
    monkeypatch.setattr(ops._lib, "call", lambda *a: pytest.fail("library touched"))
    with pytest.raises(ValueError, match=msg):
        ops.dwt_time_scale_regression(x, y, *taps, level)


def test_well_formed_cpu_calls_have_no_fallback():
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.dwt_time_scale_regression(X, X, LO, LO, LO, LO, 2)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.rows_ols(X, X)
