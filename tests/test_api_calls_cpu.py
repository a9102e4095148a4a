"""What api.py asks of the binding, characterised without a device (tests/api_calls.py): the sequence of binding calls of every
entry of the call list with the shapes, dtypes, scalars and keyword arguments they carry, the retry on the library's -5, who
closes the context, that the model is left alone, which refusal wins when two rules are broken at once, and the returned keys in
order with their shapes.  Structure only: the values belong to scripts/dbg/api_ab.py, which compares two trees bit for bit.
tests/golden/api_calls.json and the refusal table were written from the api.py before its plain / AR twins were given shared
helpers (docs/HISTORY.md A.17) and passed there as they stand."""
import json
import os
import warnings

import numpy as np
import pytest

from dynamic_factor_models_amd import _lib, api
from tests import api_calls as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "api_calls.json")) as _f:
    EXPECT = json.load(_f)
NUMERIC = (1, -5, "not positive definite")
SAMPLER = (1, -5, "Gibbs sampler: the Cholesky factor of a regression's precision does not exist")
REFUSED = (1, -3, "invalid argument")                    # a status no function answers with another call
IDS = [c.id for c in ac.CALLS]


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():                      # the stub's fills are no estimates: logs and divisions complain
        warnings.simplefilter("ignore")
        yield


def _equal(a, b):
    """Two recorded arguments, element for element."""
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return type(a) is type(b) and a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_equal(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_equal(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and a == b


def test_the_list_covers_both_families_and_the_table():
    assert list(EXPECT) == IDS and len(set(IDS)) == len(IDS)
    family = ("forecast", "filter_states", "evaluate_forecasts", "draw_paths", "simulate", "estimate_bayesian", "news")
    fns = {c.fn for c in ac.CALLS}
    assert fns >= set(family) | {f + "_ar_idio" for f in family} | {"structural_irf", "historical_decomposition", "evaluate_forecasts_rolling"}
    assert {c.fn for c in ac.FAMILIES} == ac.RETRIES | ac.NO_RETRY - {"smooth_factors_ar_idio"}
    assert not ac.RETRIES & ac.NO_RETRY and ac.GIBBS_FUNCTIONS <= ac.RETRIES
    assert {r.fn for r in ac.REFUSALS} == {c.fn for c in ac.FAMILIES} - {"structural_irf_signs", "structural_irf_proxy"}
    for fn in {r.fn for r in ac.REFUSALS}:
        assert sum(r.fn == fn for r in ac.REFUSALS) >= 3, fn


@pytest.mark.parametrize("call", ac.CALLS, ids=IDS)
def test_call_sequence_and_returned_keys(call):
    rec = ac.run(call)
    assert rec.error is None
    assert [ac.call_text(e) for e in rec.log] == EXPECT[call.id]["calls"]
    assert ac.result_text(rec.result) == EXPECT[call.id]["result"]
    assert rec.closed == 0                                                              # a context handed in is never closed
    for name, args, kw in rec.log if call in ac.FAMILIES else ():
        if "may_have_missing" in kw:                                                    # "the panel has a NaN": the new vintage of news
            panel = args[1] if name.startswith("news") else args[0]
            assert kw["may_have_missing"] is bool(np.isnan(panel).any()), name
        assert "singular_q" not in kw or kw["singular_q"] is False


@pytest.mark.parametrize("call", ac.FAMILIES, ids=[c.id for c in ac.FAMILIES])
def test_minus_five_is_retried_once_in_covariance_form_or_not_at_all(call):
    base = ac.run(call)
    rec = ac.run(call, fail=NUMERIC)
    first = base.log[0]
    if call.fn in ac.RETRIES:
        assert rec.error is None
        assert [e[0] for e in rec.log] == [first[0]] + [e[0] for e in base.log]         # exactly one call more
        again = rec.log[1]
        assert _equal(rec.log[0], first) and _equal(again[1], first[1])                 # the arrays element for element
        assert _equal({k: v for k, v in again[2].items() if k != "singular_q"}, {k: v for k, v in first[2].items() if k != "singular_q"})
        assert again[2]["singular_q"] is True and first[2].get("singular_q", False) is False
        assert sum(n != "dfm_last_error" for n, _ in rec.lib) == sum(n != "dfm_last_error" for n, _ in base.lib) + 1
        assert ac.result_text(rec.result) == ac.result_text(base.result)
    else:
        assert call.fn in ac.NO_RETRY
        assert isinstance(rec.error, _lib.DfmError) and rec.error.code == -5 and "not positive definite" in str(rec.error)
        assert len(rec.log) == 1 and _equal(rec.log[0], first)
        assert [n for n, _ in rec.lib if n != "dfm_last_error"] == [base.lib[0][0]]


@pytest.mark.parametrize("call", [c for c in ac.CALLS if c.id.startswith("estimate[")], ids=lambda c: c.id)
def test_estimate_retries_its_em_in_covariance_form(call):
    base = ac.run(call)
    n = sum(name != "dfm_last_error" for name, _ in base.lib)                           # the EM is the last library call
    rec = ac.run(call, fail=(n, -5, "not positive definite"))
    assert rec.error is None and [e[0] for e in rec.log] == [e[0] for e in base.log] + [base.log[-1][0]]
    first, again = rec.log[-2], rec.log[-1]
    assert first[0] in ("em_batch_host", "em_varp_batch_host") and _equal(first, base.log[-1]) and _equal(again[1], first[1])
    assert "singular_q" not in first[2] and again[2] == dict(first[2], singular_q=True)
    assert _equal(rec.model_after["em_params"], ac.run(call, fail=(n, -5, "not positive definite")).model_after["em_params"])


@pytest.mark.parametrize("call", [c for c in ac.FAMILIES if c.fn in ac.GIBBS_FUNCTIONS], ids=lambda c: c.id)
def test_the_samplers_own_failure_is_not_retried(call):
    rec = ac.run(call, fail=SAMPLER)
    assert isinstance(rec.error, _lib.DfmError) and rec.error.code == -5 and "Gibbs sampler" in str(rec.error)
    assert len(rec.log) == 1 and _equal(rec.log[0], ac.run(call).log[0])
    assert sum(n != "dfm_last_error" for n, _ in rec.lib) == 1


@pytest.mark.parametrize("call", ac.CALLS, ids=IDS)
def test_a_context_api_made_is_closed_exactly_once(call):
    rec = ac.run(call, own=True)
    assert rec.error is None and rec.closed == 1
    assert [ac.call_text(e) for e in rec.log] == EXPECT[call.id]["calls"]
    failed = ac.run(call, own=True, fail=REFUSED)                                       # also when the call raises
    assert isinstance(failed.error, _lib.DfmError) and failed.error.code == -3 and failed.closed == 1
    handed = ac.run(call, fail=REFUSED)
    assert isinstance(handed.error, _lib.DfmError) and handed.closed == 0 and len(handed.log) == 1


def test_a_context_is_closed_when_the_body_raises_something_else():
    class Broken:
        def __init__(self):
            self.closed = []

        def close(self):
            self.closed.append(1)

        def __getattr__(self, name):
            if name.endswith("_host"):
                raise KeyError(name)
            raise AttributeError(name)
    for call in ac.FAMILIES:
        rec = ac.run(call, own=True, ctx=Broken())
        assert isinstance(rec.error, KeyError) and rec.closed == 1, call.id
        rec = ac.run(call, ctx=Broken())
        assert isinstance(rec.error, KeyError) and rec.closed == 0, call.id


@pytest.mark.parametrize("call", [c for c in ac.CALLS if not c.mutates], ids=lambda c: c.id)
def test_the_model_is_not_modified(call):
    for fail in (None, NUMERIC):
        rec = ac.run(call, fail=fail)
        assert _equal(rec.model_before, rec.model_after)


@pytest.mark.parametrize("i", range(len(ac.REFUSALS)), ids=[f"{r.fn}-{i}" for i, r in enumerate(ac.REFUSALS)])
def test_the_refusal_that_wins_and_no_device_before_it(i, monkeypatch):
    r = ac.REFUSALS[i]
    monkeypatch.setattr(api, "_own", lambda ctx: pytest.fail("a context was asked for"))
    e = ac.refuse(r)                                                                    # its context raises AssertionError when touched
    assert type(e) is ValueError and r.wins in str(e), (r.fn, r.wins, e)


def test_draw_paths_ar_idio_takes_the_closed_interval_and_the_others_do_not():
    """The one function whose quantiles may be 0 (its message says [0, 1]); every other one refuses 0."""
    call = next(c for c in ac.CALLS if c.id == "draw_paths_ar_idio/quantiles")
    assert ac.run(call).error is None and 0.0 in call.build(ac.MODELS["ar"]())[1]["quantiles"]
    refused = {r.fn for r in ac.REFUSALS if "(0, 1]" in r.wins}
    assert refused == {"forecast", "filter_states", "evaluate_forecasts", "estimate_bayesian", "news", "structural_irf",
                       "forecast_ar_idio", "evaluate_forecasts_ar_idio", "estimate_bayesian_ar_idio", "news_ar_idio"}
