"""What api.py asks of the binding, recorded without a device: the stand-in for the loaded library (Recorder), a DfmContext on it
whose host entries log their arguments and whose outputs are deterministic fills, three hand-made models, the list of calls
that tests/test_api_calls_cpu.py characterises and scripts/dbg/api_ab.py runs under two trees, and the table of refusals.
No test functions here.  The package is taken from sys.path as it stands, so the A/B script can load this file under another tree."""
import contextlib
import ctypes
from collections import namedtuple

import numpy as np

from dynamic_factor_models_amd import _lib, api, kalman

HANDLE = 0xD0F0


class Recorder:
    """Stands for the loaded library: every dfm_* attribute is a function that stores (name, args) and returns 0
    (dfm_profile_read: 0 for index 0 only, so that the reader's loop ends).  fail=(n, code, text): the n-th call (from 1;
    dfm_last_error does not count) returns `code`, and dfm_last_error answers `text`."""

    def __init__(self, fail=None):
        self.calls = []
        self.fail = fail
        self.count = 0

    def __getattr__(self, name):
        if not name.startswith("dfm_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, args))
            if name == "dfm_last_error":
                return (self.fail[2] if self.fail else "").encode()
            self.count += 1
            if self.fail is not None and self.count == self.fail[0]:
                return self.fail[1]
            return 1 if name == "dfm_profile_read" and args[1] > 0 else 0
        return fn


def snap(x):
    """A copy of an argument that later writes cannot reach: arrays copied, containers rebuilt."""
    if isinstance(x, np.ndarray):
        return x.copy()
    if isinstance(x, dict):
        return {k: snap(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(snap(v) for v in x)
    return x


def make_ctx(fail=None):
    """A DfmContext made with __new__ on a Recorder.  Every *_host entry first appends (name, copies of the positional arguments,
    copies of the keyword arguments) to ctx.log; ctx.closed counts close().  Use it inside `stubbed()`."""
    cls = type("StubContext", (kalman.DfmContext,), dict(__del__=lambda self: None, close=lambda self: self.closed.append(1)))
    ctx = cls.__new__(cls)
    ctx._lib, ctx._h, ctx._torch, ctx._use_torch_stream, ctx.device = Recorder(fail), ctypes.c_void_p(HANDLE), None, False, 0
    ctx.log, ctx.closed = [], []
    for name in dir(kalman.DfmContext):
        if name.endswith("_host") and not isinstance(kalman.DfmContext.__dict__.get(name), staticmethod):
            def entry(*args, _name=name, _fn=getattr(kalman.DfmContext, name), **kw):
                ctx.log.append((_name, snap(args), snap(kw)))
                return _fn(ctx, *args, **kw)
            setattr(ctx, name, entry)
    return ctx


@contextlib.contextmanager
def stubbed(ctx=None):
    """While it lasts: the host backend's outputs (and the np.empty outputs of kalman.py's older entries) are fills seeded by their
    running index and shape (float64 in [0.5, 1.5), int32 in 1..3), a failed call reads its text from `ctx`'s Recorder and not from
    the library, and kalman.DfmContext() -- what api._own constructs -- hands out `ctx` (None: constructing one is an
    AssertionError)."""
    n = [0]

    def out(*shape, int32=False):
        n[0] += 1
        g = np.random.default_rng([n[0], *shape])
        return g.integers(1, 4, shape, dtype=np.int32) if int32 else g.random(shape) + 0.5

    class FilledNumpy:
        """numpy as kalman.py sees it: the older entries (PCA, ALS, OLS, quantiles, Chow) take their outputs from np.empty."""

        def __getattr__(self, name):
            return getattr(np, name)

        @staticmethod
        def empty(shape, dtype=np.float64):
            return out(*np.atleast_1d(shape).tolist(), int32=np.dtype(dtype) == np.int32)

    def made(*a, **k):
        if ctx is None:
            raise AssertionError("a context was constructed")
        return ctx
    saved = _lib.load, kalman.DfmContext
    kalman._NP.out, kalman.DfmContext, kalman.np = out, made, FilledNumpy()
    if ctx is not None:
        _lib.load = lambda: ctx._lib
    try:
        yield
    finally:
        del kalman._NP.out                                              # the class's own again
        _lib.load, kalman.DfmContext = saved
        kalman.np = np


class NoDevice:
    """A context no refusal may reach."""

    def __getattr__(self, name):
        raise AssertionError("the device was reached: " + name)


# ---------------------------------------------------------------------------------------------------- the models
def plain_model(p=1, fit=True, replicates=True, nfac_o=0):
    """A hand-made parametric fit: N = 6, 40 rows, window 3..34, r = 2, VAR(p); key A for p = 1, Avar (and A beside it in the
    replicates, as estimate() leaves them) for p = 2; three replicate parameter sets.  p = 1 has NaN cells inside the window,
    p = 2 only on the ragged edge past lastperiod."""
    g = np.random.default_rng(10 + p)
    N, r = 6, 2
    data = g.standard_normal((40, N))
    if p == 1:
        data[7, 1] = data[20, 4] = data[3, 0] = np.nan
    data[36:, 2] = np.nan
    data[38:, 5] = np.nan
    m = api.DFMModel(data, np.ones(N, dtype=int), 10, 10, 3, 34, nfac_o, r, 1e-8, 1, p)
    if not fit:
        return m
    k = r * p

    def one(g):
        A = 0.3 * g.standard_normal((r, k))
        Q = np.eye(r) + 0.1 * np.ones((r, r))
        d = dict(Lam=g.standard_normal((N, r)), R=g.random(N) + 0.5, Q=Q, mu0=np.zeros(k), P0=np.eye(k) + 0.05)
        d["A" if p == 1 else "Avar"] = A
        return d
    m.em_params = one(g)
    if replicates:
        sets = [one(g) for _ in range(3)]
        rp = {key: np.stack([s[key] for s in sets]) for key in sets[0]}
        if p > 1:
            rp["A"] = rp["Avar"]
        m.replicates = dict(params=rp)
    return m


def ar_model(n_uarlag=2, estimated=True):
    """A hand-made model with AR(2) idiosyncratic terms and a VAR(2) with constant, as estimate(m, NonParametric()) leaves one:
    N = 8, 60 rows, window 3..50, r = 2; NaN cells only on the ragged edge."""
    g = np.random.default_rng(3)
    data = g.standard_normal((60, 8))
    data[57:, 2] = np.nan
    data[58:, 5] = np.nan
    m = api.DFMModel(data, np.ones(8, dtype=int), 20, 3, 3, 50, 0, 2, 1e-8, n_uarlag, 2)
    if not estimated:
        return m
    r, p, N = m.nfac_u, m.factor_var_model.nlag, 8
    m.factor[:] = g.standard_normal(m.factor.shape)
    m.lambda_[:] = g.standard_normal((N, r))
    m.uar_coef[:] = 0.2 * g.standard_normal((N, n_uarlag))
    m.uar_ser[:] = g.random(N) + 0.5
    var = m.factor_var_model
    var.betahat = 0.1 * g.standard_normal((r * p + 1, r))
    var.seps = np.eye(r)
    return m


def ar_params(m, S=3):
    """S parameter sets in the layout of estimate_bayesian_ar_idio's `params`: the model's own, perturbed."""
    g = np.random.default_rng(4)
    inputs = api._ar_model_inputs(m)[0]
    return {k: np.stack([inputs[k] * (1.0 + 0.01 * g.random(inputs[k].shape)) for _ in range(S)]) for k in api._AR_PARAM_NAMES}


def ar_vintages(m):
    """(old, new) edge-shaped on every series: new is the data through row 55, old lacks its last two rows in four series."""
    old = m.data[:55].copy()
    old[53:, :4] = np.nan
    return old, 55


MODELS = dict(p1=lambda: plain_model(1), p2=lambda: plain_model(2), p1_bare=lambda: plain_model(1, replicates=False),
              p1_unfit=lambda: plain_model(1, fit=False), obs_unfit=lambda: plain_model(1, fit=False, nfac_o=1),
              obs=lambda: plain_model(1, nfac_o=1), ar=ar_model, ar5=lambda: ar_model(5), ar_raw=lambda: ar_model(2, estimated=False))

# ---------------------------------------------------------------------------------------------------- the calls
# id, model (a key of MODELS), function of api, build(m) -> (args, kwargs) without ctx, and whether the call writes into the model
Call = namedtuple("Call", "id model fn build mutates", defaults=(False,))
GIBBS = dict(chains=2, burn=2, thin=1)
PLAIN_TARGETS = [(0, 36), (2, 38), (5, 41)]
AR_TARGETS = [(0, 55), (5, 57)]
INSTRUMENT = np.random.default_rng(8).standard_normal(40)
RESTRICTIONS = [(0, 0, 0, 1, 1), (3, 1, 0, 0, -1)]


def _plain_calls(k):
    c = lambda name, fn, build: Call(f"{fn}[{k}]/{name}", k, fn, build)
    return [
        c("default", "forecast", lambda m: ((3,), {})),
        c("H=0", "forecast", lambda m: ((0,), {})),
        c("through", "forecast", lambda m: ((3,), dict(through=38))),
        c("quantiles", "forecast", lambda m: ((3,), dict(quantiles=[0.1, 0.9]))),
        c("default", "filter_states", lambda m: ((), {})),
        c("through", "filter_states", lambda m: ((), dict(through=40))),
        c("quantiles", "filter_states", lambda m: ((), dict(quantiles=0.5))),
        c("default", "evaluate_forecasts", lambda m: ((2,), {})),
        c("through", "evaluate_forecasts", lambda m: ((2,), dict(through=38, first_origin=12))),
        c("quantiles", "evaluate_forecasts", lambda m: ((2,), dict(quantiles=[0.25, 1.0]))),
        c("default", "draw_paths", lambda m: ((4,), {})),
        c("through", "draw_paths", lambda m: ((4, 2), dict(through=38, seed=7, first_draw=3))),
        c("parameter_draws", "draw_paths", lambda m: ((2, 1), dict(parameter_draws=True))),
        c("default", "simulate", lambda m: ((3,), {})),
        c("unmasked", "simulate", lambda m: ((3,), dict(masked=False, seed=11))),
        c("default", "estimate_bayesian", lambda m: ((4,), dict(GIBBS))),
        c("quantiles", "estimate_bayesian", lambda m: ((4,), dict(GIBBS, quantiles=[0.05, 0.95], keep_factors=True, seed=5))),
        c("default", "news", lambda m: ((34, 38, PLAIN_TARGETS), {})),
        c("arrays", "news", lambda m: ((m.data[:35].copy(), m.data[:39].copy(), PLAIN_TARGETS[:1]), {})),
        c("groups", "news", lambda m: ((34, 38, PLAIN_TARGETS), dict(groups={"a": [0, 1], "b": 5}))),
        c("quantiles", "news", lambda m: ((34, 38, PLAIN_TARGETS), dict(quantiles=[0.1, 0.9], groups={"a": [2]}))),
        c("default", "structural_irf", lambda m: ((4,), {})),
        c("named", "structural_irf", lambda m: ((4,), dict(named=[4, 1], cumulate=[0, 2], unit_effect=True, fevd=False))),
        c("quantiles", "structural_irf", lambda m: ((4,), dict(named=[4, 1], quantiles=[0.1, 0.9]))),
        c("default", "structural_irf_signs", lambda m: ((4, RESTRICTIONS), dict(candidates=16))),
        c("quantiles", "structural_irf_signs", lambda m: ((4, RESTRICTIONS), dict(candidates=16, keep=2, named=[4, 1], quantiles=[0.5]))),
        c("default", "structural_irf_proxy", lambda m: ((4, INSTRUMENT), dict(norm=1))),
        c("quantiles", "structural_irf_proxy", lambda m: ((4, INSTRUMENT), dict(norm=1, draws=5, quantiles=[0.1, 0.9]))),
        c("parameter_draws", "structural_irf_proxy",
          lambda m: ((4, INSTRUMENT), dict(norm=1, draws=5, quantiles=[0.1, 0.9], parameter_draws=True, cumulate=[3]))),
        c("default", "historical_decomposition", lambda m: ((), {})),
        c("through", "historical_decomposition", lambda m: ((), dict(through=39, named=[1, 4]))),
        c("default", "evaluate_forecasts_rolling", lambda m: ((2, 16), {})),
        c("origins", "evaluate_forecasts_rolling", lambda m: ((1, 16), dict(origins=[20, 25, 34], lags=[0, 1, 0, 2, 0, 0], max_em_iter=3))),
    ]


def _ar_calls():
    c = lambda name, fn, build: Call(f"{fn}/{name}", "ar", fn, build)
    return [
        c("default", "forecast_ar_idio", lambda m: ((3,), {})),
        c("H=0", "forecast_ar_idio", lambda m: ((0,), {})),
        c("through", "forecast_ar_idio", lambda m: ((3,), dict(through=60))),
        c("quantiles", "forecast_ar_idio", lambda m: ((3,), dict(params=ar_params(m), quantiles=[0.1, 0.9]))),
        c("default", "filter_states_ar_idio", lambda m: ((), {})),
        c("through", "filter_states_ar_idio", lambda m: ((), dict(through=58))),
        c("params", "filter_states_ar_idio", lambda m: ((), dict(params=ar_params(m, 1)))),
        c("default", "evaluate_forecasts_ar_idio", lambda m: ((2,), {})),
        c("through", "evaluate_forecasts_ar_idio", lambda m: ((2,), dict(through=58, first_origin=20))),
        c("params", "evaluate_forecasts_ar_idio", lambda m: ((2,), dict(params=ar_params(m)))),
        c("quantiles", "evaluate_forecasts_ar_idio", lambda m: ((2,), dict(params=ar_params(m), quantiles=[0.25, 1.0]))),
        c("default", "draw_paths_ar_idio", lambda m: ((4,), {})),
        c("through", "draw_paths_ar_idio", lambda m: ((4, 2), dict(through=58, seed=7, first_draw=3))),
        c("quantiles", "draw_paths_ar_idio", lambda m: ((4, 1), dict(quantiles=[0.0, 0.5, 1.0]))),
        c("params", "draw_paths_ar_idio", lambda m: ((2, 1), dict(params=ar_params(m), quantiles=[0.5]))),
        c("one draw", "draw_paths_ar_idio", lambda m: ((1,), {})),
        c("default", "simulate_ar_idio", lambda m: ((3,), {})),
        c("unmasked", "simulate_ar_idio", lambda m: ((3,), dict(masked=False, seed=11))),
        c("default", "estimate_bayesian_ar_idio", lambda m: ((4,), dict(GIBBS))),
        c("quantiles", "estimate_bayesian_ar_idio", lambda m: ((4,), dict(GIBBS, quantiles=[0.05, 0.95], keep_factors=True, seed=5))),
        c("default", "news_ar_idio", lambda m: ((*ar_vintages(m), AR_TARGETS), {})),
        c("groups", "news_ar_idio", lambda m: ((*ar_vintages(m), AR_TARGETS), dict(groups={"a": [0, 1], "b": 5}))),
        c("params", "news_ar_idio", lambda m: ((*ar_vintages(m), AR_TARGETS), dict(params=ar_params(m)))),
        c("quantiles", "news_ar_idio", lambda m: ((*ar_vintages(m), AR_TARGETS), dict(params=ar_params(m), quantiles=[0.1, 0.9], groups={"a": [2]}))),
        c("default", "smooth_factors_ar_idio", lambda m: ((), {})),
    ]


def _mf_panel():
    g = np.random.default_rng(21)
    x = g.standard_normal((36, 5))
    x[:, 3:][np.arange(36) % 3 != 2] = np.nan
    return x, ["m", "m", "m", "q_flow", "q_avg"]


def _mf_fit(nrep):
    """What estimate_mixed_frequency returns, made by hand (r = 2, p = 1, L = 5)."""
    g = np.random.default_rng(22)
    x, w = _mf_panel()
    k = 2 * 5
    one = lambda: dict(Lam=g.standard_normal((5, 2)), R=g.random(5) + 0.5, Avar=0.3 * g.standard_normal((2, 2)), Q=np.eye(2),
                       mu0=np.zeros(k), P0=np.eye(k))
    fit = dict(one(), W=api.mf_weights(w, 5), mean=np.nanmean(x, axis=0), sd=np.nanstd(x, axis=0))
    if nrep:
        sets = [one() for _ in range(nrep)]
        fit["replicates"] = dict(params={key: np.stack([s[key] for s in sets]) for key in sets[0]})
    return fit


def _other_calls():
    """The callers of the context manager outside the two families; most of them write into the model (a fresh one per call)."""
    w = lambda id, model, fn, build: Call(id, model, fn, build, True)
    return [
        w("estimate[p1]", "p1_unfit", "estimate", lambda m: ((), dict(max_em_iter=4))),
        w("estimate[p2]", "p1_unfit", "estimate", lambda m: ((), dict(max_em_iter=4, factor_lags=2))),
        w("estimate/nonparametric", "ar_raw", "estimate", lambda m: ((api.NonParametric(),), {})),
        w("estimate_factor", "ar_raw", "estimate_factor", lambda m: ((), dict(max_iter=5))),
        w("estimate_factor_loading", "ar", "estimate_factor_loading", lambda m: ((), {})),
        w("estimate_ar_idio", "ar", "estimate_ar_idio", lambda m: ((), dict(max_em_iter=4))),
        Call("estimate_factor_numbers", "ar_raw", "estimate_factor_numbers", lambda m: (([1, 2],), {})),
        Call("estimate_factor_numbers/aw", "ar", "estimate_factor_numbers", lambda m: (([1, 2],), dict(with_aw=True))),
        Call("amengual_watson_test", "ar", "amengual_watson_test", lambda m: ((), {})),
        Call("break_tests", "ar", "break_tests", lambda m: ((30,), dict(min_obs=20))),
        Call("estimate_mixed_frequency", "p1", "estimate_mixed_frequency", lambda m: ((*_mf_panel(), 2, 1), dict(max_em_iter=3))),
        Call("forecast_mixed", "p1", "forecast_mixed", lambda m: ((_mf_fit(0), _mf_panel()[0], 2), {})),
        Call("forecast_mixed/quantiles", "p1", "forecast_mixed", lambda m: ((_mf_fit(3), _mf_panel()[0], 2, [0.1, 0.9]), {})),
    ]


# estimate_mixed_frequency and forecast_mixed take no model
NO_MODEL = {"estimate_mixed_frequency", "forecast_mixed"}
# the VAR(2) fit differs from the VAR(1) one in where A comes from and in the state's width: its richest variants are enough
_P2_VARIANTS = ("through", "quantiles", "parameter_draws", "unmasked", "origins")
CALLS = (_plain_calls("p1") + [c for c in _plain_calls("p2") if c.id.split("/")[1] in _P2_VARIANTS] + _ar_calls() + _other_calls())
FAMILIES = [c for c in CALLS if not c.mutates and c.fn not in ("estimate_factor_numbers", "amengual_watson_test", "break_tests",
                                                               "estimate_mixed_frequency", "forecast_mixed", "smooth_factors_ar_idio")]
# the functions that answer the library's -5 (DFM_E_NUMERIC) with one more call in covariance form, and those that do not
RETRIES = {"forecast", "draw_paths", "estimate_bayesian", "news", "historical_decomposition", "evaluate_forecasts_rolling",
           "structural_irf_proxy", "draw_paths_ar_idio", "estimate_bayesian_ar_idio", "news_ar_idio"}
NO_RETRY = {"filter_states", "evaluate_forecasts", "simulate", "structural_irf", "structural_irf_signs", "forecast_ar_idio",
            "filter_states_ar_idio", "evaluate_forecasts_ar_idio", "simulate_ar_idio", "smooth_factors_ar_idio"}
GIBBS_FUNCTIONS = {"estimate_bayesian", "estimate_bayesian_ar_idio"}

Record = namedtuple("Record", "log lib result error closed model_before model_after")


def model_state(m):
    """Everything of a model a call could write into, copied."""
    keys = ("data", "factor", "lambda_", "uar_coef", "uar_ser", "r2")
    s = {k: getattr(m, k).copy() for k in keys}
    var = m.factor_var_model
    s.update({"var." + k: np.array(getattr(var, k)) for k in ("betahat", "seps", "M", "Q", "G", "resid")})
    s["em_params"] = snap(m.em_params)
    s["replicates"] = snap(getattr(m, "replicates", None))
    return s


def run(call, own=False, fail=None, ctx=None):
    """One call of the list on a fresh model and a fresh stub context (`ctx`: that one instead): what the binding was asked, what
    came back (or the exception), how often the context was closed.  own: the call gets no ctx and api._own constructs the stub."""
    m = MODELS[call.model]()
    args, kw = call.build(m)
    ctx = make_ctx(fail) if ctx is None else ctx
    before = model_state(m)
    result = error = None
    lead = () if call.fn in NO_MODEL else (m,)
    with stubbed(ctx if own or isinstance(ctx, kalman.DfmContext) else None):
        try:
            result = getattr(api, call.fn)(*lead, *args, **(kw if own else dict(kw, ctx=ctx)))
        except Exception as e:                                          # the record keeps it: the caller decides what it means
            error = e
    lib = [(n, tuple(a for a in ar if type(a) in (int, float))) for n, ar in getattr(getattr(ctx, "_lib", None), "calls", [])]
    return Record(getattr(ctx, "log", []), lib, result, error, len(getattr(ctx, "closed", [])), before, model_state(m))


# ---------------------------------------------------------------------------------------------------- the refusals
# function, model, build(m) -> (args, kwargs): an input that breaks two rules at once; `wins`: a piece of the message that is raised
Refusal = namedtuple("Refusal", "fn model build wins")
_BAD_PARAMS = {"Lam": 0}
_GAP = lambda m: (lambda old: (old.__setitem__((30, 6), np.nan), old)[1])(ar_vintages(m)[0].copy())
REFUSALS = [
    Refusal("forecast", "p1_unfit", lambda m: ((-1,), {}), "H must be >= 0"),
    Refusal("forecast", "p1_unfit", lambda m: ((3,), dict(through=99)), "has not been estimated"),
    Refusal("forecast", "obs", lambda m: ((3,), dict(through=99)), "forecast needs nfac_o = 0"),
    Refusal("forecast", "p1", lambda m: ((3,), dict(through=99, quantiles=[2.0])), "through must lie in lastperiod..T (34..40)"),
    Refusal("forecast", "p1_bare", lambda m: ((3,), dict(quantiles=[2.0])), "quantile bands need bootstrap replicates"),
    Refusal("forecast", "p1", lambda m: ((0,), dict(quantiles=[2.0])), "quantile bands need H >= 1"),
    Refusal("forecast", "p1", lambda m: ((3,), dict(quantiles=[0.0])), "quantiles must lie in (0, 1]"),
    Refusal("filter_states", "p1_unfit", lambda m: ((), dict(through=99)), "has not been estimated"),
    Refusal("filter_states", "p1", lambda m: ((), dict(through=99, quantiles=[2.0])), "through must lie"),
    Refusal("filter_states", "p1_bare", lambda m: ((), dict(quantiles=[2.0])), "quantile bands need bootstrap replicates"),
    Refusal("filter_states", "p1", lambda m: ((), dict(quantiles=[])), "quantiles must lie in (0, 1]"),
    Refusal("evaluate_forecasts", "p1_unfit", lambda m: ((0,), {}), "H must be >= 1"),
    Refusal("evaluate_forecasts", "p1", lambda m: ((2,), dict(through=99, first_origin=0)), "through must lie"),
    Refusal("evaluate_forecasts", "p1", lambda m: ((2,), dict(quantiles=[0.0], first_origin=0)), "quantiles must lie in (0, 1]"),
    Refusal("evaluate_forecasts", "p1", lambda m: ((2,), dict(first_origin=0)), "first_origin must lie in initperiod..through (3..34)"),
    Refusal("draw_paths", "p1", lambda m: ((0, -1), {}), "ndraws must be >= 1"),
    Refusal("draw_paths", "p1_unfit", lambda m: ((2,), dict(first_draw=-1)), "first_draw must be >= 0"),
    Refusal("draw_paths", "p1_bare", lambda m: ((2,), dict(through=99, parameter_draws=True)), "through must lie"),
    Refusal("draw_paths", "p1_bare", lambda m: ((2,), dict(parameter_draws=True)), "parameter draws need bootstrap replicates"),
    Refusal("simulate", "p1_unfit", lambda m: ((0,), {}), "ndraws must be >= 1"),
    Refusal("simulate", "obs_unfit", lambda m: ((2,), {}), "has not been estimated"),
    Refusal("simulate", "obs", lambda m: ((2,), {}), "simulate needs nfac_o = 0"),
    Refusal("estimate_bayesian", "p1_unfit", lambda m: ((4,), dict(chains=0)), "ndraws >= 1, chains >= 1"),
    Refusal("estimate_bayesian", "p1_unfit", lambda m: ((4,), dict(quantiles=[2.0])), "has not been estimated"),
    Refusal("estimate_bayesian", "p1", lambda m: ((4,), dict(quantiles=[2.0], prior={"bogus": 1})), "quantiles must lie in (0, 1]"),
    Refusal("estimate_bayesian", "p1", lambda m: ((4,), dict(prior={"bogus": 1})), "unknown prior entries"),
    Refusal("news", "p1_unfit", lambda m: ((34, 38, []), {}), "has not been estimated"),
    Refusal("news", "p1", lambda m: ((99, 38, []), {}), "old vintage: through must lie"),
    Refusal("news", "p1", lambda m: ((34, 38, []), dict(groups={"g": [9]})), "at least one target"),
    Refusal("news", "p1", lambda m: ((34, 38, [(9, 36)]), dict(groups={"g": [9]})), "target column 9 is not one of the series estimate() used"),
    Refusal("news", "p1_bare", lambda m: ((34, 38, PLAIN_TARGETS), dict(groups={"g": [9]}, quantiles=[0.5])),
            "groups['g'] must list columns estimate() used"),
    Refusal("news", "p1_bare", lambda m: ((34, 38, PLAIN_TARGETS), dict(quantiles=[2.0])), "quantile bands need bootstrap replicates"),
    Refusal("news", "p1", lambda m: ((34, 38, PLAIN_TARGETS), dict(quantiles=[2.0])), "quantiles must lie in (0, 1]"),
    Refusal("structural_irf", "p1_unfit", lambda m: ((0,), {}), "H must be >= 1"),
    Refusal("structural_irf", "p1", lambda m: ((4,), dict(unit_effect=True, quantiles=[2.0])), "unit_effect needs named series"),
    Refusal("structural_irf", "p1_bare", lambda m: ((4,), dict(quantiles=[2.0])), "quantile bands need named series"),
    Refusal("structural_irf", "p1_bare", lambda m: ((4,), dict(named=[77], quantiles=[2.0])), "quantile bands need bootstrap replicates"),
    Refusal("structural_irf", "p1", lambda m: ((4,), dict(named=[77], quantiles=[2.0])), "quantiles must lie in (0, 1]"),
    Refusal("structural_irf", "p1", lambda m: ((4,), dict(named=[77])), "named: series 77 is not among the series estimate() used"),
    Refusal("historical_decomposition", "p1_unfit", lambda m: ((), dict(through=99)), "has not been estimated"),
    Refusal("historical_decomposition", "p1", lambda m: ((), dict(through=99, named=[0])), "through must lie"),
    Refusal("historical_decomposition", "p1", lambda m: ((), dict(named=[0, 0])), "named must be 2 distinct series"),
    Refusal("evaluate_forecasts_rolling", "p1_unfit", lambda m: ((-1, 16), {}), "H must be >= 0"),
    Refusal("evaluate_forecasts_rolling", "p1_unfit", lambda m: ((2, 1), {}), "has not been estimated"),
    Refusal("evaluate_forecasts_rolling", "p1", lambda m: ((2, 1), dict(step=0)), "window must lie in 2..32"),
    Refusal("evaluate_forecasts_rolling", "p1", lambda m: ((2, 16), dict(step=0, origins=[1])), "step must be >= 1"),
    Refusal("forecast_ar_idio", "ar5", lambda m: ((-1,), {}), "H must be >= 0"),
    Refusal("forecast_ar_idio", "ar5", lambda m: ((3,), dict(through=99)), "forecast_ar_idio needs 1 <= n_uarlag <= 4"),
    Refusal("forecast_ar_idio", "ar", lambda m: ((3,), dict(through=99, params=_BAD_PARAMS)), "through must lie in lastperiod..T (50..60)"),
    Refusal("forecast_ar_idio", "ar", lambda m: ((0,), dict(quantiles=[2.0])), "quantile bands need parameter sets"),
    Refusal("forecast_ar_idio", "ar", lambda m: ((0,), dict(quantiles=[2.0], params=_BAD_PARAMS)), "quantile bands need H >= 1"),
    Refusal("forecast_ar_idio", "ar", lambda m: ((3,), dict(quantiles=[2.0], params=_BAD_PARAMS)), "quantiles must lie in (0, 1]"),
    Refusal("forecast_ar_idio", "ar_raw", lambda m: ((3,), dict(params=_BAD_PARAMS)), "params serve the quantile bands"),
    Refusal("forecast_ar_idio", "ar_raw", lambda m: ((3,), dict(quantiles=[0.5], params=_BAD_PARAMS)), "factor_var_model is not estimated"),
    Refusal("forecast_ar_idio", "ar", lambda m: ((3,), dict(quantiles=[0.5], params=_BAD_PARAMS)), "params lacks"),
    Refusal("filter_states_ar_idio", "ar5", lambda m: ((), dict(through=99)), "filter_states_ar_idio needs 1 <= n_uarlag <= 4"),
    Refusal("filter_states_ar_idio", "ar", lambda m: ((), dict(through=99, params=_BAD_PARAMS)), "through must lie"),
    Refusal("filter_states_ar_idio", "ar_raw", lambda m: ((), dict(params=_BAD_PARAMS)), "factor_var_model is not estimated"),
    Refusal("filter_states_ar_idio", "ar", lambda m: ((), dict(params=ar_params(m))), "takes one parameter set"),
    Refusal("evaluate_forecasts_ar_idio", "ar5", lambda m: ((0,), {}), "H must be >= 1"),
    Refusal("evaluate_forecasts_ar_idio", "ar", lambda m: ((2,), dict(quantiles=[2.0], through=99)), "quantile bands need parameter sets"),
    Refusal("evaluate_forecasts_ar_idio", "ar5", lambda m: ((2,), dict(quantiles=[2.0], params=_BAD_PARAMS)), "quantiles must lie in (0, 1]"),
    Refusal("evaluate_forecasts_ar_idio", "ar5", lambda m: ((2,), dict(through=99)), "evaluate_forecasts_ar_idio needs 1 <= n_uarlag <= 4"),
    Refusal("evaluate_forecasts_ar_idio", "ar", lambda m: ((2,), dict(through=99, first_origin=0)), "through must lie"),
    Refusal("evaluate_forecasts_ar_idio", "ar", lambda m: ((2,), dict(params=_BAD_PARAMS, first_origin=0)), "params lacks"),
    Refusal("evaluate_forecasts_ar_idio", "ar", lambda m: ((2,), dict(first_origin=0)), "first_origin must lie in initperiod + n_uarlag..through (5..50)"),
    Refusal("simulate_ar_idio", "ar5", lambda m: ((0,), {}), "ndraws must be >= 1"),
    Refusal("simulate_ar_idio", "ar5", lambda m: ((2,), {}), "simulate_ar_idio needs 1 <= n_uarlag <= 4"),
    Refusal("simulate_ar_idio", "ar_raw", lambda m: ((2,), {}), "factor_var_model is not estimated"),
    Refusal("draw_paths_ar_idio", "ar", lambda m: ((0, -1), {}), "ndraws must be >= 1"),
    Refusal("draw_paths_ar_idio", "ar5", lambda m: ((2,), dict(quantiles=[2.0])), "draw_paths_ar_idio needs 1 <= n_uarlag <= 4"),
    Refusal("draw_paths_ar_idio", "ar", lambda m: ((2,), dict(quantiles=[1.5], through=99)), "quantiles must lie in [0, 1]"),
    Refusal("draw_paths_ar_idio", "ar", lambda m: ((2,), dict(quantiles=[np.nan])), "quantiles must lie in [0, 1]"),
    Refusal("draw_paths_ar_idio", "ar", lambda m: ((20000,), dict(quantiles=[0.0], through=99)), "bands need ndraws <= 16384"),
    Refusal("draw_paths_ar_idio", "ar", lambda m: ((2,), dict(quantiles=[0.0], through=99, params=_BAD_PARAMS)), "through must lie"),
    Refusal("draw_paths_ar_idio", "ar_raw", lambda m: ((2,), dict(params=_BAD_PARAMS)), "factor_var_model is not estimated"),
    Refusal("draw_paths_ar_idio", "ar", lambda m: ((2,), dict(params=_BAD_PARAMS)), "params lacks"),
    Refusal("estimate_bayesian_ar_idio", "ar5", lambda m: ((4,), dict(thin=0)), "ndraws >= 1, chains >= 1"),
    Refusal("estimate_bayesian_ar_idio", "ar5", lambda m: ((4,), dict(quantiles=[2.0])), "estimate_bayesian_ar_idio needs 1 <= n_uarlag <= 4"),
    Refusal("estimate_bayesian_ar_idio", "ar_raw", lambda m: ((4,), dict(quantiles=[2.0])), "quantiles must lie in (0, 1]"),
    Refusal("estimate_bayesian_ar_idio", "ar_raw", lambda m: ((4,), dict(prior={"bogus": 1})), "factor_var_model is not estimated"),
    Refusal("estimate_bayesian_ar_idio", "ar", lambda m: ((4,), dict(prior={"bogus": 1})), "unknown prior entries"),
    Refusal("news_ar_idio", "ar5", lambda m: ((*ar_vintages(m), []), {}), "news_ar_idio needs 1 <= n_uarlag <= 4"),
    Refusal("news_ar_idio", "ar", lambda m: ((ar_vintages(m)[0], 99, []), {}), "new vintage: through must lie"),
    Refusal("news_ar_idio", "ar_raw", lambda m: ((*ar_vintages(m), []), {}), "at least one target"),
    Refusal("news_ar_idio", "ar", lambda m: ((*ar_vintages(m), [(9, 55)]), dict(groups={"g": [9]})),
            "target column 9 is not one of the series the model uses"),
    Refusal("news_ar_idio", "ar", lambda m: ((*ar_vintages(m), [(0, 4)]), dict(groups={"g": [9]})), "conditioning values"),
    Refusal("news_ar_idio", "ar", lambda m: ((*ar_vintages(m), AR_TARGETS), dict(groups={"g": [9]}, params=_BAD_PARAMS)),
            "groups['g'] must list columns the model uses"),
    Refusal("news_ar_idio", "ar", lambda m: ((*ar_vintages(m), AR_TARGETS), dict(params=_BAD_PARAMS, quantiles=[2.0])), "params lacks"),
    Refusal("news_ar_idio", "ar", lambda m: ((_GAP(m), 55, AR_TARGETS), dict(quantiles=[2.0])), "quantile bands need parameter sets"),
    Refusal("news_ar_idio", "ar", lambda m: ((_GAP(m), 55, AR_TARGETS), dict(quantiles=[2.0], params=ar_params(m))), "quantiles must lie in (0, 1]"),
    Refusal("news_ar_idio", "ar", lambda m: ((_GAP(m), 55, AR_TARGETS), {}), "vintage: "),
]


def refuse(r):
    """The exception refusal `r` ends in, with a context that no refusal may reach."""
    m = MODELS[r.model]()
    args, kw = r.build(m)
    with stubbed():
        try:
            getattr(api, r.fn)(m, *args, ctx=NoDevice(), **kw)
        except Exception as e:
            return e
    return None


# ---------------------------------------------------------------------------------------------------- a record as text
def _sig(x):
    """Shape and kind of a value, values of scalars: f[2,3] a float64 array, i / i4 integers, b booleans."""
    if isinstance(x, np.ndarray):
        kind = {"float64": "f", "int64": "i", "int32": "i4", "bool": "b", "uint8": "u1"}.get(str(x.dtype), str(x.dtype))
        return kind + str(list(x.shape)).replace(" ", "")
    if isinstance(x, dict):
        return "{" + " ".join(f"{k}={_sig(v)}" for k, v in x.items()) + "}"
    if isinstance(x, (np.floating, np.integer, np.bool_)):
        return f"{type(x).__name__}({x})"
    return repr(x).replace(" ", "")


def call_text(entry):
    """One logged binding call as one line: name, positional arguments, keyword arguments in call order."""
    name, args, kw = entry
    return " ".join([name] + [_sig(a) for a in args] + ["|"] + [f"{k}={_sig(v)}" for k, v in kw.items()])


def result_text(result):
    """A returned value's keys in order with shapes; scalars by type only (their values belong to the A/B script)."""
    def leaf(v):
        if isinstance(v, dict):
            return "{" + " ".join(f"{k}:{leaf(x)}" for k, x in v.items()) + "}"
        if isinstance(v, np.ndarray):
            return _sig(v)
        if isinstance(v, (list, tuple)):
            return type(v).__name__ + "(" + " ".join(leaf(x) for x in v) + ")"
        return type(v).__name__
    return leaf(result)
