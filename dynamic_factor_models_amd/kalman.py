"""Host-side wrappers of the C-ABI (include/dfm_hip.h) over torch device tensors / NumPy arrays.

torch is plumbing only (device memory, the current HIP stream, torch.distributed); every number is
produced by the hand-written gfx950 kernels inside libdfmhip.so.

Each kind of entry (smoother pass, EM, forecast, path draws, news) has ONE marshalling body; the model families are the
rows of a table and the two sides of the boundary (device tensors / host arrays) are two backends.
"""
from __future__ import annotations

import ctypes
from collections import namedtuple
from typing import Optional

import numpy as np

from . import _lib


def _check(h, rc: int):
    if rc != 0:
        raise _lib.DfmError(rc, _lib.load().dfm_last_error(h).decode())


def _ptr(a):
    """Pointer to a NumPy array's data.  None (an output not asked for) AND a zero-size array (rho with q = 0) give null."""
    return None if a is None or a.size == 0 else ctypes.c_void_p(a.ctypes.data)


def _ids(device_ids):
    return None if device_ids is None else np.ascontiguousarray(device_ids, dtype=np.int32)


def _flags(may_have_missing, singular_q=False, be=None, panel=None):
    """The flags word of a call.  may_have_missing None: backend `be` scans `panel` for a NaN."""
    if may_have_missing is None:
        may_have_missing = be.has_nan(panel)
    return (_lib.DFM_F_MAY_HAVE_MISSING if may_have_missing else 0) | (_lib.DFM_F_SINGULAR_Q if singular_q else 0)


# ---------------------------------------------------------------------- the two marshalling backends
# A backend says how an input becomes a pointer (inp, then ptr), how a parameter the library updates does (upd, then ptr),
# how an output is made (out) and whether the panel has a NaN (has_nan).  raw: the pointer of an int32 array, unchecked.
class _Numpy:
    """Host-pointer entries: read-only inputs as C-ordered float64 (no copy if they are), updated parameters as a copy (the
    caller's arrays stay untouched), outputs from np.empty.  No type or shape checks."""
    suffix = ""

    def inp(self, a):
        return np.ascontiguousarray(a, dtype=np.float64)

    def upd(self, a):
        return np.array(a, dtype=np.float64, order="C", copy=True)

    def out(self, *shape, int32=False):
        return np.empty(shape, dtype=np.int32 if int32 else np.float64)

    def inp_bytes(self, a):
        return None if a is None else np.ascontiguousarray(np.asarray(a) != 0, dtype=np.uint8)

    def has_nan(self, panel):
        return bool(np.isnan(panel).any())

    def ptr(self, a, name=None, shape=None):
        return _ptr(a)

    raw = ptr_bytes = ptr

    def sync(self):
        pass


class _Torch:
    """Device-pointer entries of context `ctx`: tensors pass as they are (parameters are updated IN PLACE), pointers through
    ctx._dev with its type, contiguity and shape checks, outputs from torch.empty on the panel's device; sync hands torch's
    current stream to the handle before the call."""
    suffix = "_dev"

    def __init__(self, ctx, panel):
        self.ctx, self.torch, self.panel = ctx, ctx._torch, panel

    def inp(self, t):
        return t

    upd = inp_bytes = inp

    def out(self, *shape, int32=False):
        return self.torch.empty(shape, dtype=self.torch.int32 if int32 else self.torch.float64, device=self.panel.device)

    @staticmethod
    def has_nan(panel):                 # static: a body that marshals by hand asks _Torch itself
        return bool(panel.isnan().any().item())

    def ptr(self, t, name, shape=None):
        """As _ptr: None and a zero-size tensor (rho with q = 0) give null, unchecked."""
        return None if t is None or 0 in t.shape else self.ctx._dev(t, name, shape)

    def ptr_bytes(self, t, name, shape=None):
        """A mask: a contiguous uint8 tensor on the device (None: null)."""
        if t is None:
            return None
        if not isinstance(t, self.torch.Tensor) or not t.is_cuda or t.dtype != self.torch.uint8 or not t.is_contiguous():
            raise TypeError(f"{name}: expected a contiguous uint8 tensor on the HIP device")
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name}: shape {tuple(t.shape)} != expected {tuple(shape)}")
        return ctypes.c_void_p(t.data_ptr())

    def raw(self, t):
        return ctypes.c_void_p(t.data_ptr())

    def sync(self):
        self.ctx._sync_stream()


_NP = _Numpy()


# ---------------------------------------------------------------------- the four model families
# infix: dfm_ks_pass<infix>_batch[_dev] and dfm_em<infix>_batch[_dev];  names: the parameter arrays after the panel, in call order;
# readonly: those EM does not update (the host EM neither copies nor returns them);  bytes: those that are byte masks, not float64
# (always read only; None passes as null);  geom(B, T, N, r, *arrays) gives, from the
# arrays' shapes, (the extra integer arguments, the rows of f_smooth / P_smooth, the expected shape of each array); k in it is
# the state width.
_Family = namedtuple("_Family", "infix names readonly geom bytes", defaults=((),))


def _geom_plain(B, T, N, r, Lam, R, A, Q, mu0, P0):
    k = r
    return (), T, ((B, N, r), (B, N), (B, r, r), (B, r, r), (B, k), (B, k, k))


def _geom_varp(B, T, N, r, Lam, R, Avar, Q, mu0, P0):
    k = Avar.shape[2]
    p = k // r
    return (p,), T, ((B, N, r), (B, N), (B, r, r * p), (B, r, r), (B, k), (B, k, k))


def _geom_ar(B, T, N, r, Lam, sig2, rho, Avar, Q, mu0, P0):
    p, q = Avar.shape[2] // r, rho.shape[2]
    k = r * max(p, q + 1)
    return (p, q), T - q, ((B, N, r), (B, N), (B, N, q), (B, r, r * p), (B, r, r), (B, k), (B, k, k))


def _geom_mf(B, T, N, r, Lam, R, W, Avar, Q, mu0, P0):
    p, L = Avar.shape[2] // r, W.shape[1]
    k = r * max(p, L)
    return (p, L), T, ((B, N, r), (B, N), (N, L), (B, r, r * p), (B, r, r), (B, k), (B, k, k))


def _geom_mf_blocks(B, T, N, r, Lam, R, W, free, Avar, Q, mu0, P0):
    extra, rows, sh = _geom_mf(B, T, N, r, Lam, R, W, Avar, Q, mu0, P0)
    return extra, rows, sh[:3] + ((N, r),) + sh[3:]


_PLAIN = _Family("", ("Lam", "R", "A", "Q", "mu0", "P0"), (), _geom_plain)
_VARP = _Family("_varp", ("Lam", "R", "Avar", "Q", "mu0", "P0"), (), _geom_varp)
_AR = _Family("_ar", ("Lam", "sig2", "rho", "Avar", "Q", "mu0", "P0"), (), _geom_ar)
_MF = _Family("_mf", ("Lam", "R", "W", "Avar", "Q", "mu0", "P0"), ("W",), _geom_mf)
_MF_BLOCKS = _Family("_mf_blocks", ("Lam", "R", "W", "free", "Avar", "Q", "mu0", "P0"), ("W", "free"), _geom_mf_blocks, ("free",))
# Differences between the public wrappers that nobody chose.  They are kept as they were; the next change can decide them:
#  - want_P exists on ks_pass_batch_host only; the varp / ar / mf host passes always return P_smooth;
#  - ks_pass_batch_multi_host has no singular_q and never sets DFM_F_SINGULAR_Q (em_obs_batch_host: neither);
#  - only the device path checks shapes (of the parameters, mean and sd); the host path checks none.


def _model(fam, be, panel, params, update=False):
    """The panel and the parameter arrays of family `fam` as backend `be` takes them (update: EM will write the parameters), and
    what their shapes say: (panel, params, (B, T, N, r, *extra integers), output rows, expected shapes)."""
    panel = be.inp(panel)
    params = [(be.inp_bytes if n in fam.bytes else be.upd if update and n not in fam.readonly else be.inp)(a)
              for n, a in zip(fam.names, params)]
    B, T, N = panel.shape
    r = params[0].shape[2]
    extra, rows, shapes = fam.geom(B, T, N, r, *params)
    return panel, params, (B, T, N, r) + extra, rows, shapes


def _ptrs(be, fam, arrays, shapes):
    return [(be.ptr_bytes if n in fam.bytes else be.ptr)(a, n, s) for a, n, s in zip(arrays, fam.names, shapes)]


def _pass_out(be, B, rows, r, want_P=True):
    """(f_smooth, P_smooth or None, loglik)"""
    return be.out(B, rows, r), be.out(B, rows, r * (r + 1) // 2) if want_P else None, be.out(B)


def _em_out(be, B, rows, r, max_iter, want_smooth=True, want_P=True):
    """(loglik_path, iters, f_smooth or None, P_smooth or None): P_smooth only together with f_smooth."""
    path, iters = be.out(B, max_iter), be.out(B, int32=True)
    f = be.out(B, rows, r) if want_smooth else None
    return path, iters, f, be.out(B, rows, r * (r + 1) // 2) if (want_smooth and want_P) else None


def _pair(be, mean, sd):
    if (mean is None) != (sd is None):
        raise ValueError("mean and sd go together")
    return (None, None) if mean is None else (be.inp(mean), be.inp(sd))


class DfmMulti:
    """The library's multi-GPU object (dfm_multi, csrc/multi.hip): `ngpu` GPUs of this node driven from THIS process -- one
    handle, stream and workspace per GPU and ONE RCCL communicator, created once; the job's replicates stay resident in
    the GPUs' HBM between calls.  What a host without torch.distributed (Julia) uses; `bench.py --driver lib` times it.
    force_comm: build the (1-rank) communicator also for ngpu = 1, so that the all-gather path runs on one GPU."""

    def __init__(self, ngpu: int = 1, device_ids=None, force_comm: bool = False):
        self._lib = _lib.load()
        h = ctypes.c_void_p()
        err = ctypes.create_string_buffer(700)
        ids = _ids(device_ids)
        rc = self._lib.dfm_multi_create(ctypes.byref(h), int(ngpu), _ptr(ids),
                                        _lib.DFM_MULTI_F_FORCE_COMM if force_comm else 0, err, 700)
        if rc != 0:
            raise _lib.DfmError(rc, err.value.decode())
        self._m = h
        self.shape = None
        self._max_iter = 0

    def close(self):
        if getattr(self, "_m", None):
            self._lib.dfm_multi_destroy(self._m)
            self._m = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != 0:
            raise _lib.DfmError(rc, self._lib.dfm_multi_last_error(self._m).decode())

    @property
    def ngpu(self):
        return self._lib.dfm_multi_ngpu(self._m)

    @property
    def has_comm(self):
        return bool(self._lib.dfm_multi_has_comm(self._m))

    def load(self, panel, Lam, R, A, Q, mu0, P0):
        """Upload a job (NumPy, layouts of em_batch_host) to the GPUs that own its replicates."""
        panel, *params = map(_NP.inp, (panel, Lam, R, A, Q, mu0, P0))
        B, T, N = panel.shape
        r = params[0].shape[2]
        self._ck(self._lib.dfm_multi_load(self._m, B, T, N, r, _ptr(panel), *map(_ptr, params)))
        self.shape = (B, T, N, r)

    def synth(self, seed: int, first_replicate: int, B: int, T: int, N: int, r: int, missing_prob: float = 0.0,
              pca_start: bool = False):
        """Generate the job where it lives: GPU g draws replicates first_replicate + [lo_g, hi_g) (dfm_synth_panels_dev);
        pca_start replaces the DGP parameters by the PCA + OLS start."""
        self._ck(self._lib.dfm_multi_synth(self._m, int(seed), int(first_replicate), B, T, N, r, float(missing_prob),
                                           1 if pca_start else 0))
        self.shape = (B, T, N, r)

    def ks_pass(self, want_P: bool = True, may_have_missing: bool = False, singular_q: bool = False):
        self._ck(self._lib.dfm_multi_ks_pass(self._m, 1 if want_P else 0, _flags(may_have_missing, singular_q)))

    def em(self, max_iter: int = 10, tol: float = 0.0, want_smooth: bool = True, want_P: bool = True,
           may_have_missing: bool = False, singular_q: bool = False) -> int:
        """The EM loop on the resident job (parameters updated in place on the GPUs); returns the iterations run."""
        ran = ctypes.c_int(0)
        self._max_iter = int(max_iter)
        self._ck(self._lib.dfm_multi_em(self._m, int(max_iter), float(tol), 1 if want_smooth else 0, 1 if want_P else 0,
                                        _flags(may_have_missing, singular_q), ctypes.cast(ctypes.byref(ran), ctypes.c_void_p)))
        return ran.value

    def fetch(self, what: str):
        """One resident array of the whole job, global replicate order (NumPy)."""
        B, T, N, r = self.shape
        npk = r * (r + 1) // 2
        table = {"Lam": (_lib.DFM_MULTI_LAM, (B, N, r), np.float64), "R": (_lib.DFM_MULTI_R, (B, N), np.float64),
                 "A": (_lib.DFM_MULTI_A, (B, r, r), np.float64), "Q": (_lib.DFM_MULTI_Q, (B, r, r), np.float64),
                 "mu0": (_lib.DFM_MULTI_MU0, (B, r), np.float64), "P0": (_lib.DFM_MULTI_P0, (B, r, r), np.float64),
                 "f_smooth": (_lib.DFM_MULTI_F_SMOOTH, (B, T, r), np.float64),
                 "P_smooth": (_lib.DFM_MULTI_P_SMOOTH, (B, T, npk), np.float64),
                 "loglik": (_lib.DFM_MULTI_LOGLIK, (B,), np.float64),
                 "loglik_path": (_lib.DFM_MULTI_LOGLIK_PATH, (B, self._max_iter), np.float64),
                 "iters": (_lib.DFM_MULTI_ITERS, (B,), np.int32), "panel": (_lib.DFM_MULTI_PANEL, (B, T, N), np.float64)}
        code, shape, dt = table[what]
        out = np.empty(shape, dtype=dt)
        self._ck(self._lib.dfm_multi_fetch(self._m, code, ctypes.c_void_p(out.ctypes.data)))
        return out


class DfmContext:
    """One libdfmhip handle bound to a HIP device and (by default) torch's current stream."""

    def __init__(self, device: Optional[int] = None, use_torch_stream: bool = True):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("DfmContext needs a HIP device (torch.cuda.is_available() is False); "
                               "there is no CPU fallback for this path")
        self._lib = _lib.load()
        self.device = torch.cuda.current_device() if device is None else int(device)
        self._torch = torch
        self._use_torch_stream = bool(use_torch_stream)
        stream = torch.cuda.current_stream(self.device).cuda_stream if use_torch_stream else None
        h = ctypes.c_void_p()
        rc = self._lib.dfm_create(ctypes.byref(h), self.device, ctypes.c_void_p(stream))
        if rc != 0:
            raise _lib.DfmError(rc, "dfm_create failed")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.dfm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ helpers
    def _dev(self, t, name, shape=None):
        torch = self._torch
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float64 or not t.is_contiguous():
            raise TypeError(f"{name}: expected a contiguous float64 tensor on the HIP device")
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name}: shape {tuple(t.shape)} != expected {tuple(shape)}")
        return ctypes.c_void_p(t.data_ptr())

    def _sync_stream(self):
        if not self._use_torch_stream:      # the handle keeps the stream it created for itself
            return
        s = self._torch.cuda.current_stream(self.device).cuda_stream
        self._lib.dfm_set_stream(self._h, ctypes.c_void_p(s))

    def synchronize(self):
        """Wait for the handle's stream AND surface the status word of the last call (NaN in a panel declared balanced,
        an expired bounded wait of the one-launch pass, PCA start not converged): the device-pointer entry points only
        enqueue, so this is where their failures become exceptions."""
        _check(self._h, self._lib.dfm_synchronize(self._h))

    check_status = synchronize

    def hbm_probe(self, nbytes: int = 1 << 30, iters: int = 10):
        """dfm_hbm_probe: {"read_dma": GB/s, "copy": GB/s, "write": GB/s} of this device, measured now."""
        self._torch.cuda.synchronize(self.device)
        out = {}
        for name, mode in (("read_dma", 0), ("copy", 1), ("write", 2)):
            g = ctypes.c_double(); ms = ctypes.c_double()
            with self._torch.cuda.device(self.device):
                _check(self._h, self._lib.dfm_hbm_probe(self._h, int(nbytes), mode, int(iters), ctypes.byref(g), ctypes.byref(ms)))
            out[name] = g.value
        return out

    def chunk_fallbacks(self):
        """dfm_chunk_fallbacks: (failed, total) replicates of the last pass that ran on a time-chunked recursion (total = 0:
        it did not); `failed` of them were redone by the sequential kernel."""
        nf = ctypes.c_int(); nt = ctypes.c_int()
        _check(self._h, self._lib.dfm_chunk_fallbacks(self._h, ctypes.byref(nf), ctypes.byref(nt)))
        return nf.value, nt.value

    def profile_enable(self, on: bool = True):
        self._sync_stream()
        _check(self._h, self._lib.dfm_profile_enable(self._h, 1 if on else 0))

    def profile_read(self):
        """{kernel name: (total ms, launches)} since profile_enable(True)."""
        out = {}
        idx = 0
        while True:
            name = ctypes.create_string_buffer(64)
            ms = ctypes.c_double(); n = ctypes.c_int()
            rc = self._lib.dfm_profile_read(self._h, idx, name, 64, ctypes.byref(ms), ctypes.byref(n))
            if rc != 0:
                break
            if n.value:
                out[name.value.decode()] = (ms.value, n.value)
            idx += 1
        return out

    # ------------------------------------------------------------------ one body per kind of entry
    def _pass(self, fam, be, panel, params, want_P, may_have_missing, singular_q):
        """dfm_ks_pass<fam>_batch[_dev] through backend `be`: (f_smooth, P_smooth or None, loglik)."""
        panel, params, dims, rows, shapes = _model(fam, be, panel, params)
        flags = _flags(may_have_missing, singular_q, be, panel)
        f, P, ll = _pass_out(be, dims[0], rows, dims[3], want_P)
        be.sync()
        rc = getattr(self._lib, f"dfm_ks_pass{fam.infix}_batch{be.suffix}")(
            self._h, *dims, be.ptr(panel, "panel"), *_ptrs(be, fam, params, shapes), be.ptr(f, "f_smooth"),
            be.ptr(P, "P_smooth"), be.ptr(ll, "loglik"), flags)
        _check(self._h, rc)
        return f, P, ll

    def _em(self, fam, be, panel, params, max_iter, tol, want_smooth, want_P, may_have_missing, singular_q):
        """dfm_em<fam>_batch[_dev] through backend `be`: (updated parameters by name, loglik_path, iters, f_smooth, P_smooth).
        The device backend updates the caller's tensors in place; the host backend updates copies and returns those."""
        panel, params, dims, rows, shapes = _model(fam, be, panel, params, update=True)
        flags = _flags(may_have_missing, singular_q, be, panel)
        path, iters, f, P = _em_out(be, dims[0], rows, dims[3], max_iter, want_smooth, want_P)
        be.sync()
        rc = getattr(self._lib, f"dfm_em{fam.infix}_batch{be.suffix}")(
            self._h, *dims, be.ptr(panel, "panel"), *_ptrs(be, fam, params, shapes), int(max_iter), float(tol),
            be.ptr(path, "loglik_path"), be.raw(iters), be.ptr(f, "f_smooth"), be.ptr(P, "P_smooth"), flags)
        _check(self._h, rc)
        return {n: a for n, a in zip(fam.names, params) if n not in fam.readonly}, path, iters, f, P

    def _forecast(self, be, panel, params, H, mean, sd, want_var, want_common, want_P, may_have_missing, singular_q):
        panel, params, dims, _, shapes = _model(_VARP, be, panel, params)
        B, T, N, r, p = dims
        if int(H) < 0:
            raise ValueError("H must be >= 0")
        mean, sd = _pair(be, mean, sd)
        flags = _flags(may_have_missing, singular_q, be, panel)
        TH = T + int(H)
        xhat = be.out(B, TH, N)
        xvar = be.out(B, TH, N) if want_var else None
        common = be.out(B, TH, N) if want_common else None
        f = be.out(B, TH, r)
        P = be.out(B, TH, r * (r + 1) // 2) if want_P else None
        ll = be.out(B)
        be.sync()
        rc = getattr(self._lib, "dfm_forecast_batch" + be.suffix)(
            self._h, B, T, N, r, p, int(H), be.ptr(panel, "panel"), *_ptrs(be, _VARP, params, shapes),
            be.ptr(mean, "mean", (B, N)), be.ptr(sd, "sd", (B, N)), be.ptr(xhat, "xhat"), be.ptr(xvar, "xvar"),
            be.ptr(common, "common"), be.ptr(f, "f_out"), be.ptr(P, "P_out"), be.ptr(ll, "loglik"), flags)
        _check(self._h, rc)
        return dict(xhat=xhat, xvar=xvar, common=common, f=f, P=P, loglik=ll)

    def _simsmooth(self, be, panel, params, D, H, seed, first_draw, mean, sd, want_x, may_have_missing, singular_q):
        panel, params, dims, _, shapes = _model(_VARP, be, panel, params)
        B, T, N, r, p = dims
        if int(D) < 1:
            raise ValueError("D must be >= 1")
        if int(H) < 0:
            raise ValueError("H must be >= 0")
        mean, sd = _pair(be, mean, sd)
        flags = _flags(may_have_missing, singular_q, be, panel)
        f = be.out(B, int(D), T + int(H), r)
        x = be.out(B, int(D), T + int(H), N) if want_x else None
        be.sync()
        rc = getattr(self._lib, "dfm_simsmooth_batch" + be.suffix)(
            self._h, B, int(D), T, N, r, p, int(H), be.ptr(panel, "panel"), *_ptrs(be, _VARP, params, shapes),
            be.ptr(mean, "mean", (B, N)), be.ptr(sd, "sd", (B, N)), int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_draw),
            be.ptr(f, "f_draw"), be.ptr(x, "x_draw"), flags)
        _check(self._h, rc)
        return dict(f=f, x=x)

    def _news(self, be, old, new, params, targets, mean, sd, want_news, want_weight, may_have_missing, singular_q):
        new, params, dims, _, shapes = _model(_VARP, be, new, params)
        B, T, N, r, p = dims
        old = be.inp(old)
        if tuple(old.shape) != (B, T, N):
            raise ValueError("old and new must have the same shape")
        mean, sd = _pair(be, mean, sd)
        tt, ti = self._targets(targets, T, N)
        G = tt.size
        flags = _flags(may_have_missing, singular_q, be, new)       # the NEW vintage is the one scanned
        yhat, impact = be.out(B, 3, G), be.out(B, G, N)
        news = be.out(B, T, N) if want_news else None
        weight = be.out(B, G, T, N) if want_weight else None
        be.sync()
        rc = getattr(self._lib, "dfm_news_batch" + be.suffix)(
            self._h, B, T, N, r, p, be.ptr(old, "old"), be.ptr(new, "new"), *_ptrs(be, _VARP, params, shapes),
            be.ptr(mean, "mean", (B, N)), be.ptr(sd, "sd", (B, N)), G, _ptr(tt), _ptr(ti), be.ptr(yhat, "yhat"),
            be.ptr(impact, "impact"), be.ptr(news, "news"), be.ptr(weight, "weight"), flags)
        _check(self._h, rc)
        return dict(yhat=yhat, impact=impact, news=news, weight=weight)

    # ------------------------------------------------------------------ smoother pass
    def ks_pass_batch(self, panel, Lam, R, A, Q, mu0, P0, want_P: bool = True,
                      may_have_missing: Optional[bool] = None, out=None, singular_q: bool = False):
        """One Kalman-smoother pass per replicate (device tensors in, device tensors out).
        Returns (f_smooth [B,T,r], P_smooth [B,T,r(r+1)/2] or None, loglik [B]).  Asynchronous on
        torch's current stream."""
        B, T, N = panel.shape       # written out, not through _pass: the benchmark's timed loop issues this call (with out=)
        r = Lam.shape[2]            # every ~0.2 ms, and the table-driven body costs about twice the host time
        flags = _flags(may_have_missing, singular_q, _Torch, panel)
        f, P, ll = _pass_out(_Torch(self, panel), B, T, r, want_P) if out is None else out
        self._sync_stream()
        rc = self._lib.dfm_ks_pass_batch_dev(
            self._h, B, T, N, r, self._dev(panel, "panel"), self._dev(Lam, "Lam", (B, N, r)),
            self._dev(R, "R", (B, N)), self._dev(A, "A", (B, r, r)), self._dev(Q, "Q", (B, r, r)),
            self._dev(mu0, "mu0", (B, r)), self._dev(P0, "P0", (B, r, r)), self._dev(f, "f_smooth"),
            self._dev(P, "P_smooth") if P is not None else None, self._dev(ll, "loglik"), flags)
        _check(self._h, rc)
        return f, P, ll

    def ks_pass_batch_host(self, panel, Lam, R, A, Q, mu0, P0, want_P: bool = True,
                           may_have_missing: Optional[bool] = None, singular_q: bool = False):
        """Same through the HOST-pointer entry point (what Julia's ccall binds): NumPy in/out."""
        return self._pass(_PLAIN, _NP, panel, (Lam, R, A, Q, mu0, P0), want_P, may_have_missing, singular_q)

    # ------------------------------------------------------------------ EM
    def em_step_batch(self, panel, Lam, R, A, Q, mu0, P0, may_have_missing: Optional[bool] = None):
        """One EM iteration per replicate; parameters (device tensors) are updated IN PLACE.
        Returns loglik [B] at the parameters passed in."""
        B, T, N = panel.shape       # written out as ks_pass_batch is: a driver steps it in a loop
        r = Lam.shape[2]
        flags = _flags(may_have_missing, False, _Torch, panel)
        ll = self._torch.empty((B,), dtype=self._torch.float64, device=panel.device)
        self._sync_stream()
        rc = self._lib.dfm_em_step_batch_dev(
            self._h, B, T, N, r, self._dev(panel, "panel"), self._dev(Lam, "Lam", (B, N, r)),
            self._dev(R, "R", (B, N)), self._dev(A, "A", (B, r, r)), self._dev(Q, "Q", (B, r, r)),
            self._dev(mu0, "mu0", (B, r)), self._dev(P0, "P0", (B, r, r)), self._dev(ll, "loglik"), flags)
        _check(self._h, rc)
        return ll

    def em_batch(self, panel, Lam, R, A, Q, mu0, P0, max_iter: int = 10, tol: float = 0.0,
                 want_smooth: bool = True, want_P: bool = True, may_have_missing: Optional[bool] = None,
                 singular_q: bool = False):
        """max_iter EM iterations (parameters updated in place).  Returns
        (loglik_path [B,max_iter] (NaN past iters[b]), iters [B] int32, f_smooth, P_smooth)."""
        return self._em(_PLAIN, _Torch(self, panel), panel, (Lam, R, A, Q, mu0, P0), max_iter, tol, want_smooth, want_P,
                        may_have_missing, singular_q)[1:]

    def em_iterate_batch(self, panel, Lam, R, A, Q, mu0, P0, k: int, max_iter: int, tol: float, path, iters, active,
                         f=None, P=None, may_have_missing: Optional[bool] = False, singular_q: bool = False):
        """EM iteration number k of max_iter (dfm_em_iterate_batch_dev): parameters updated in place, bookkeeping in the
        CALLER's device tensors path [B,max_iter] f64, iters [B] i32, active [B] i32 (they persist between calls; the
        k = 0 call initialises them).  The unit a multi-GPU driver steps: shard.em_batch_sharded."""
        be = _Torch(self, panel)
        panel, params, dims, _, shapes = _model(_PLAIN, be, panel, (Lam, R, A, Q, mu0, P0))
        flags = _flags(may_have_missing, singular_q, be, panel)
        be.sync()
        rc = self._lib.dfm_em_iterate_batch_dev(
            self._h, *dims, be.ptr(panel, "panel"), *_ptrs(be, _PLAIN, params, shapes), int(k), int(max_iter), float(tol),
            be.ptr(path, "loglik_path", (dims[0], max_iter)), be.raw(iters), be.raw(active), be.ptr(f, "f_smooth"),
            be.ptr(P, "P_smooth"), flags)
        _check(self._h, rc)

    def em_batch_host(self, panel, Lam, R, A, Q, mu0, P0, max_iter: int = 10, tol: float = 0.0,
                      may_have_missing: Optional[bool] = None, singular_q: bool = False):
        """Host-pointer EM entry (what Julia's ccall binds).  Returns (params dict, loglik_path, iters,
        f_smooth, P_smooth); inputs are not modified."""
        return self._em(_PLAIN, _NP, panel, (Lam, R, A, Q, mu0, P0), max_iter, tol, True, True, may_have_missing, singular_q)

    def em_obs_batch_host(self, panel, G, Lam, R, A, Q, mu0, P0, max_iter: int = 10, tol: float = 0.0,
                          may_have_missing: Optional[bool] = None):
        """dfm_em_obs_batch: EM of the model with OBSERVED factors g_t as known regressors (include/dfm_hip.h).
        panel [B,T,N], G [B,T,r_o] (no NaN), Lam [B,N,r_o+r_u] (observed-factor loadings first), A / Q / P0 [B,r_u,r_u],
        mu0 [B,r_u].  Returns (params dict, loglik_path, iters, f_smooth [B,T,r_u], P_smooth); inputs are not modified."""
        panel, G = _NP.inp(panel), _NP.inp(G)
        Lam, R, A, Q, mu0, P0 = map(_NP.upd, (Lam, R, A, Q, mu0, P0))
        B, T, N = panel.shape
        ro = G.shape[2]
        ru = Lam.shape[2] - ro
        if G.shape[:2] != (B, T) or A.shape != (B, ru, ru):
            raise ValueError("em_obs_batch_host: G must be [B,T,r_o] and A [B,r_u,r_u] with Lam [B,N,r_o+r_u]")
        flags = _flags(may_have_missing, False, _NP, panel)
        path, iters, f, P = _em_out(_NP, B, T, ru, max_iter)
        rc = self._lib.dfm_em_obs_batch(self._h, B, T, N, ru, ro, *map(_ptr, (panel, G, Lam, R, A, Q, mu0, P0)),
                                        int(max_iter), float(tol), _ptr(path), _ptr(iters), _ptr(f), _ptr(P), flags)
        _check(self._h, rc)
        return dict(Lam=Lam, R=R, A=A, Q=Q, mu0=mu0, P0=P0), path, iters, f, P

    # ------------------------------------------------------------------ several GPUs from one process (multi.hip)
    @staticmethod
    def em_batch_multi_host(ngpu, panel, Lam, R, A, Q, mu0, P0, max_iter: int = 10, tol: float = 0.0,
                            may_have_missing: Optional[bool] = None, device_ids=None, singular_q: bool = False):
        """dfm_em_batch_multi: the EM loop on `ngpu` GPUs from THIS process (one host thread per GPU, library-owned
        RCCL communicator, one all-gather of {loglik, active} per iteration) -- what the Julia host binds.  NumPy in /
        out as em_batch_host; also returns the number of iterations every GPU ran."""
        lib = _lib.load()
        panel, params, dims, rows, _ = _model(_PLAIN, _NP, panel, (Lam, R, A, Q, mu0, P0), update=True)
        flags = _flags(may_have_missing, singular_q, _NP, panel)
        path, iters, f, P = _em_out(_NP, dims[0], rows, dims[3], max_iter)
        ids, ran, err = _ids(device_ids), ctypes.c_int(0), ctypes.create_string_buffer(700)
        rc = lib.dfm_em_batch_multi(int(ngpu), _ptr(ids), *dims, _ptr(panel), *map(_ptr, params), int(max_iter), float(tol),
                                    _ptr(path), _ptr(iters), _ptr(f), _ptr(P), flags,
                                    ctypes.cast(ctypes.byref(ran), ctypes.c_void_p), err, 700)
        if rc != 0:
            raise _lib.DfmError(rc, err.value.decode())
        return dict(zip(_PLAIN.names, params)), path, iters, f, P, ran.value

    @staticmethod
    def ks_pass_batch_multi_host(ngpu, panel, Lam, R, A, Q, mu0, P0, may_have_missing: Optional[bool] = None,
                                 device_ids=None):
        """dfm_ks_pass_batch_multi: the smoother pass with the replicates split over `ngpu` GPUs (no exchange)."""
        lib = _lib.load()
        panel, params, dims, rows, _ = _model(_PLAIN, _NP, panel, (Lam, R, A, Q, mu0, P0))
        flags = _flags(may_have_missing, False, _NP, panel)
        f, P, ll = _pass_out(_NP, dims[0], rows, dims[3])
        ids, err = _ids(device_ids), ctypes.create_string_buffer(700)
        rc = lib.dfm_ks_pass_batch_multi(int(ngpu), _ptr(ids), *dims, _ptr(panel), *map(_ptr, params), _ptr(f), _ptr(P),
                                         _ptr(ll), flags, err, 700)
        if rc != 0:
            raise _lib.DfmError(rc, err.value.decode())
        return f, P, ll

    # ------------------------------------------------------------------ VAR(p) factor dynamics (companion form)
    def ks_pass_varp_batch(self, panel, Lam, R, Avar, Q, mu0, P0, want_P: bool = True,
                           may_have_missing: Optional[bool] = None, singular_q: bool = False):
        """Smoother pass of x_t = Lam f_t + e_t, f_t = A_1 f_{t-1} + .. + A_p f_{t-p} + eta_t (device tensors).
        Avar [B,r,r p] = [A_1 .. A_p], Q [B,r,r], mu0 [B,r p], P0 [B,r p,r p].  Returns (f_smooth, P_smooth, loglik).
        singular_q (here and in the other VAR(p) / AR entry points): the r x r block Q itself may be rank deficient -- DFM_F_SINGULAR_Q,
        the kernels that never invert it (include/dfm_hip.h)."""
        return self._pass(_VARP, _Torch(self, panel), panel, (Lam, R, Avar, Q, mu0, P0), want_P, may_have_missing, singular_q)

    def em_varp_batch(self, panel, Lam, R, Avar, Q, mu0, P0, max_iter: int = 10, tol: float = 0.0,
                      want_smooth: bool = True, want_P: bool = True, may_have_missing: Optional[bool] = None, singular_q: bool = False):
        """EM for the VAR(p) model, parameters (device tensors) updated in place.
        Returns (loglik_path [B,max_iter], iters [B] int32, f_smooth, P_smooth)."""
        return self._em(_VARP, _Torch(self, panel), panel, (Lam, R, Avar, Q, mu0, P0), max_iter, tol, want_smooth, want_P,
                        may_have_missing, singular_q)[1:]

    def em_varp_batch_host(self, panel, Lam, R, Avar, Q, mu0, P0, max_iter: int = 10, tol: float = 0.0,
                           may_have_missing: Optional[bool] = None, singular_q: bool = False):
        """Host-pointer entry (what Julia's ccall binds).  Returns (params dict, loglik_path, iters, f_smooth,
        P_smooth); inputs are not modified."""
        return self._em(_VARP, _NP, panel, (Lam, R, Avar, Q, mu0, P0), max_iter, tol, True, True, may_have_missing, singular_q)

    def ks_pass_varp_batch_host(self, panel, Lam, R, Avar, Q, mu0, P0, may_have_missing: Optional[bool] = None, singular_q: bool = False):
        return self._pass(_VARP, _NP, panel, (Lam, R, Avar, Q, mu0, P0), True, may_have_missing, singular_q)

    # ------------------------------------------------------------------ nowcasts and forecasts (forecast.hip)
    def forecast_batch(self, panel, Lam, R, Avar, Q, mu0, P0, H: int, mean=None, sd=None, want_var: bool = True,
                       want_common: bool = True, want_P: bool = True, may_have_missing: Optional[bool] = None,
                       singular_q: bool = False):
        """dfm_forecast_batch_dev (device tensors, torch's current stream): smoothed / forecast moments and the panel's
        nowcasts over T + H rows.  Avar [B,r,r p] ([A_1 .. A_p]; p = 1: A), Q [B,r,r], mu0 [B,r p], P0 [B,r p,r p];
        mean / sd [B,N] (both or neither) put the outputs into data units.  Returns dict(xhat, xvar, common [B,T+H,N],
        f [B,T+H,r], P [B,T+H,r(r+1)/2], loglik [B]); the outputs not asked for are None."""
        return self._forecast(_Torch(self, panel), panel, (Lam, R, Avar, Q, mu0, P0), H, mean, sd, want_var, want_common, want_P,
                              may_have_missing, singular_q)

    def forecast_batch_host(self, panel, Lam, R, Avar, Q, mu0, P0, H: int, mean=None, sd=None, want_var: bool = True,
                            want_common: bool = True, want_P: bool = True, may_have_missing: Optional[bool] = None,
                            singular_q: bool = False):
        """dfm_forecast_batch (host pointers; what Julia's ccall binds): NumPy in / out, same dict as forecast_batch."""
        return self._forecast(_NP, panel, (Lam, R, Avar, Q, mu0, P0), H, mean, sd, want_var, want_common, want_P,
                              may_have_missing, singular_q)

    # ------------------------------------------------------------------ posterior path draws (simsmooth.hip)
    def simsmooth_batch(self, panel, Lam, R, Avar, Q, mu0, P0, D: int, H: int = 0, seed: int = 0, first_draw: int = 0,
                        mean=None, sd=None, want_x: bool = True, may_have_missing: Optional[bool] = None,
                        singular_q: bool = False):
        """dfm_simsmooth_batch_dev (device tensors, torch's current stream): D joint posterior draws per replicate of the factor
        path and of the missing / future cells over T + H rows (include/dfm_hip.h).  Avar [B,r,r p] ([A_1 .. A_p]), Q [B,r,r],
        mu0 [B,r p], P0 [B,r p,r p]; mean / sd [B,N] (both or neither) put x into data units.  Returns dict(f [B,D,T+H,r],
        x [B,D,T+H,N] or None)."""
        return self._simsmooth(_Torch(self, panel), panel, (Lam, R, Avar, Q, mu0, P0), D, H, seed, first_draw, mean, sd, want_x,
                               may_have_missing, singular_q)

    def simsmooth_batch_host(self, panel, Lam, R, Avar, Q, mu0, P0, D: int, H: int = 0, seed: int = 0, first_draw: int = 0,
                             mean=None, sd=None, want_x: bool = True, may_have_missing: Optional[bool] = None,
                             singular_q: bool = False):
        """dfm_simsmooth_batch (host pointers; what Julia's ccall binds): NumPy in / out, same dict as simsmooth_batch."""
        return self._simsmooth(_NP, panel, (Lam, R, Avar, Q, mu0, P0), D, H, seed, first_draw, mean, sd, want_x,
                               may_have_missing, singular_q)

    # ------------------------------------------------------------------ news decomposition of nowcast revisions (news.hip)
    @staticmethod
    def _targets(targets, T, N):
        tg = np.ascontiguousarray(np.asarray(targets, dtype=np.int64).reshape(-1, 2))
        if tg.shape[0] < 1:
            raise ValueError("at least one target is needed")
        if np.any(tg[:, 0] < 0) or np.any(tg[:, 1] < 0) or np.any(tg[:, 1] >= N):
            raise ValueError("targets are (row t* >= 0, column 0 <= i* < N) pairs")
        return np.ascontiguousarray(tg[:, 0], dtype=np.int32), np.ascontiguousarray(tg[:, 1], dtype=np.int32)

    def news_batch(self, old, new, Lam, R, Avar, Q, mu0, P0, targets, mean=None, sd=None, want_news: bool = True,
                   want_weight: bool = True, may_have_missing: Optional[bool] = None, singular_q: bool = False):
        """dfm_news_batch_dev (device tensors, torch's current stream): the news decomposition of the revision of G target cells
        between two vintages old / new [B,T,N] (include/dfm_hip.h).  targets: G (row t*, column i*) pairs, 0-based, host side;
        Avar [B,r,r p], Q [B,r,r], mu0 [B,r p], P0 [B,r p,r p]; mean / sd [B,N] (both or neither) put the outputs into data
        units.  Returns dict(yhat [B,3,G] (old, revised, new), impact [B,G,N], news [B,T,N] or None, weight [B,G,T,N] or None);
        the status word (DFM_E_VINTAGE) is read by synchronize()."""
        return self._news(_Torch(self, new), old, new, (Lam, R, Avar, Q, mu0, P0), targets, mean, sd, want_news, want_weight,
                          may_have_missing, singular_q)

    def news_batch_host(self, old, new, Lam, R, Avar, Q, mu0, P0, targets, mean=None, sd=None, want_news: bool = True,
                        want_weight: bool = True, may_have_missing: Optional[bool] = None, singular_q: bool = False):
        """dfm_news_batch (host pointers; what Julia's ccall binds): NumPy in / out, same dict as news_batch."""
        return self._news(_NP, old, new, (Lam, R, Avar, Q, mu0, P0), targets, mean, sd, want_news, want_weight,
                          may_have_missing, singular_q)

    # ------------------------------------------------------------------ AR idiosyncratic terms (quasi-differencing)
    def ks_pass_ar_batch(self, panel, Lam, sig2, rho, Avar, Q, mu0, P0, want_P: bool = True,
                         may_have_missing: Optional[bool] = None, singular_q: bool = False):
        """Smoother pass with AR(q) idiosyncratic terms (rho [B,N,q], sig2 [B,N]: the reference's uar_coef, uar_ser^2)
        and VAR(p) factors (Avar [B,r,r p]); mu0 [B,r m], P0 [B,r m,r m], m = max(p, q+1).  Device tensors.
        Returns (f_smooth [B,T-q,r], P_smooth or None, loglik [B]) for rows q+1..T."""
        return self._pass(_AR, _Torch(self, panel), panel, (Lam, sig2, rho, Avar, Q, mu0, P0), want_P, may_have_missing, singular_q)

    def ks_pass_ar_batch_host(self, panel, Lam, sig2, rho, Avar, Q, mu0, P0, may_have_missing: Optional[bool] = None, singular_q: bool = False):
        """Host-pointer entry (what Julia's ccall binds)."""
        return self._pass(_AR, _NP, panel, (Lam, sig2, rho, Avar, Q, mu0, P0), True, may_have_missing, singular_q)

    def em_ar_batch(self, panel, Lam, sig2, rho, Avar, Q, mu0, P0, max_iter: int = 10, tol: float = 0.0,
                    want_smooth: bool = True, want_P: bool = True, may_have_missing: Optional[bool] = None, singular_q: bool = False):
        """Joint ECM estimation with AR(q) idiosyncratic terms (include/dfm_hip.h: dfm_em_ar_batch_dev).  Device tensors;
        Lam [B,N,r], sig2 [B,N], rho [B,N,q], Avar [B,r,r p], Q, mu0 [B,r m], P0 [B,r m,r m] are UPDATED IN PLACE.
        Returns (loglik_path [B,max_iter], iters [B], f_smooth [B,T-q,r] or None, P_smooth or None)."""
        return self._em(_AR, _Torch(self, panel), panel, (Lam, sig2, rho, Avar, Q, mu0, P0), max_iter, tol, want_smooth, want_P,
                        may_have_missing, singular_q)[1:]

    def em_ar_batch_host(self, panel, Lam, sig2, rho, Avar, Q, mu0, P0, max_iter: int = 10, tol: float = 0.0,
                         may_have_missing: Optional[bool] = None, singular_q: bool = False):
        """Host-pointer entry (what Julia's ccall binds).  Returns (params dict, loglik_path, iters, f_smooth, P_smooth);
        inputs are not modified."""
        return self._em(_AR, _NP, panel, (Lam, sig2, rho, Avar, Q, mu0, P0), max_iter, tol, True, True, may_have_missing,
                        singular_q)

    # ------------------------------------------------------------------ mixed frequency (monthly factors, quarterly series)
    def ks_pass_mf_batch(self, panel, Lam, R, W, Avar, Q, mu0, P0, want_P: bool = True,
                         may_have_missing: Optional[bool] = None, singular_q: bool = False):
        """Smoother pass of the mixed-frequency model (include/dfm_hip.h: dfm_ks_pass_mf_batch_dev): series i loads on
        sum_l W[i,l] f_{t-l}; W [N,L] is shared by the batch; mu0 [B,r m], P0 [B,r m,r m], m = max(p, L).  Device tensors.
        Returns (f_smooth [B,T,r], P_smooth or None, loglik [B])."""
        return self._pass(_MF, _Torch(self, panel), panel, (Lam, R, W, Avar, Q, mu0, P0), want_P, may_have_missing, singular_q)

    def ks_pass_mf_batch_host(self, panel, Lam, R, W, Avar, Q, mu0, P0, may_have_missing: Optional[bool] = None, singular_q: bool = False):
        """Host-pointer entry (what Julia's ccall binds)."""
        return self._pass(_MF, _NP, panel, (Lam, R, W, Avar, Q, mu0, P0), True, may_have_missing, singular_q)

    def em_mf_batch(self, panel, Lam, R, W, Avar, Q, mu0, P0, max_iter: int = 10, tol: float = 0.0,
                    want_smooth: bool = True, want_P: bool = True, may_have_missing: Optional[bool] = None, singular_q: bool = False):
        """EM estimation of the mixed-frequency model (include/dfm_hip.h: dfm_em_mf_batch_dev).  Device tensors; Lam [B,N,r],
        R [B,N], Avar [B,r,r p], Q, mu0 [B,r m], P0 [B,r m,r m] are UPDATED IN PLACE; W [N,L] is read only.
        Returns (loglik_path [B,max_iter], iters [B], f_smooth [B,T,r] or None, P_smooth or None)."""
        return self._em(_MF, _Torch(self, panel), panel, (Lam, R, W, Avar, Q, mu0, P0), max_iter, tol, want_smooth, want_P,
                        may_have_missing, singular_q)[1:]

    def em_mf_batch_host(self, panel, Lam, R, W, Avar, Q, mu0, P0, max_iter: int = 10, tol: float = 0.0,
                         may_have_missing: Optional[bool] = None, singular_q: bool = False):
        """Host-pointer entry (what Julia's ccall binds).  Returns (params dict, loglik_path, iters, f_smooth, P_smooth);
        inputs are not modified."""
        return self._em(_MF, _NP, panel, (Lam, R, W, Avar, Q, mu0, P0), max_iter, tol, True, True, may_have_missing,
                        singular_q)

    def em_mf_blocks_batch_dev(self, panel, Lam, R, W, free, Avar, Q, mu0, P0, max_iter: int = 10, tol: float = 0.0,
                               want_smooth: bool = True, want_P: bool = True, may_have_missing: Optional[bool] = None,
                               singular_q: bool = False):
        """em_mf_batch with fixed loadings (include/dfm_hip.h, the blocks twin of dfm_em_mf_batch_dev).  free [N,r]: a uint8
        device tensor, nonzero = estimated; a fixed entry of Lam keeps the value it has on entry; the mask is read only.  None:
        em_mf_batch itself.  Returns (loglik_path [B,max_iter], iters [B], f_smooth [B,T,r] or None, P_smooth or None)."""
        return self._em(_MF_BLOCKS, _Torch(self, panel), panel, (Lam, R, W, free, Avar, Q, mu0, P0), max_iter, tol, want_smooth,
                        want_P, may_have_missing, singular_q)[1:]

    def em_mf_blocks_batch_host(self, panel, Lam, R, W, free, Avar, Q, mu0, P0, max_iter: int = 10, tol: float = 0.0,
                                may_have_missing: Optional[bool] = None, singular_q: bool = False):
        """Host-pointer entry (what Julia's ccall binds); free [N,r]: any array, nonzero = estimated.  Returns (params dict,
        loglik_path, iters, f_smooth, P_smooth); inputs are not modified."""
        return self._em(_MF_BLOCKS, _NP, panel, (Lam, R, W, free, Avar, Q, mu0, P0), max_iter, tol, True, True, may_have_missing,
                        singular_q)

    # ------------------------------------------------------------------ PCA initialisation / synthetic panels
    def pca_init_batch(self, panel, r: int, want_factors: bool = True):
        """PCA + OLS start of EM on balanced standardised panels (device tensor [B,T,N], no NaN).
        Returns (Lam, R, A, Q, mu0, P0, factors or None) as device tensors.  Asynchronous."""
        torch = self._torch
        B, T, N = panel.shape
        f64 = dict(dtype=torch.float64, device=panel.device)
        Lam = torch.empty((B, N, r), **f64); R = torch.empty((B, N), **f64)
        A = torch.empty((B, r, r), **f64); Q = torch.empty((B, r, r), **f64)
        mu0 = torch.empty((B, r), **f64); P0 = torch.empty((B, r, r), **f64)
        F = torch.empty((B, T, r), **f64) if want_factors else None
        self._sync_stream()
        rc = self._lib.dfm_pca_init_batch_dev(
            self._h, B, T, N, int(r), self._dev(panel, "panel"), self._dev(Lam, "Lam"), self._dev(R, "R"),
            self._dev(A, "A"), self._dev(Q, "Q"), self._dev(mu0, "mu0"), self._dev(P0, "P0"),
            self._dev(F, "factors") if F is not None else None)
        _check(self._h, rc)
        return Lam, R, A, Q, mu0, P0, F

    def pca_init_batch_host(self, panel, r: int):
        """Host-pointer PCA entry (what Julia's ccall binds): NumPy in / out."""
        panel = _NP.inp(panel)
        B, T, N = panel.shape
        Lam = np.empty((B, N, r)); R = np.empty((B, N)); A = np.empty((B, r, r)); Q = np.empty((B, r, r))
        mu0 = np.empty((B, r)); P0 = np.empty((B, r, r)); F = np.empty((B, T, r))
        rc = self._lib.dfm_pca_init_batch(self._h, B, T, N, int(r), *map(_ptr, (panel, Lam, R, A, Q, mu0, P0, F)))
        _check(self._h, rc)
        return dict(Lam=Lam, R=R, A=A, Q=Q, mu0=mu0, P0=P0), F

    def synth_panels(self, seed: int, first_replicate: int, B: int, T: int, N: int, r: int,
                     missing_prob: float = 0.0):
        """Synthetic replicates of the SURVEY §8(d) DGP generated on the device.  Returns
        (panel [B,T,N], (Lam, R, A, Q, mu0, P0)) -- the DGP parameters rescaled to the standardised panel."""
        torch = self._torch
        dev = torch.device("cuda", self.device)
        f64 = dict(dtype=torch.float64, device=dev)
        panel = torch.empty((B, T, N), **f64)
        Lam = torch.empty((B, N, r), **f64); R = torch.empty((B, N), **f64)
        A = torch.empty((B, r, r), **f64); Q = torch.empty((B, r, r), **f64)
        mu0 = torch.empty((B, r), **f64); P0 = torch.empty((B, r, r), **f64)
        self._sync_stream()
        rc = self._lib.dfm_synth_panels_dev(
            self._h, ctypes.c_uint64(seed), ctypes.c_int64(first_replicate), B, T, N, r,
            ctypes.c_double(missing_prob), self._dev(panel, "panel"), self._dev(Lam, "Lam"), self._dev(R, "R"),
            self._dev(A, "A"), self._dev(Q, "Q"), self._dev(mu0, "mu0"), self._dev(P0, "P0"))
        _check(self._h, rc)
        return panel, (Lam, R, A, Q, mu0, P0)

    # ------------------------------------------------------------------ non-parametric estimator (als.hip)
    def als_batch_host(self, z, F0, r_each=None, nt_min: int = 20, max_iter: int = 10 ** 8, tol: float = 1e-8,
                       path_cap: int = 0, want_R2: bool = False, shared_panel: Optional[bool] = None):
        """Batched `estimate_factor!` sweeps (dfm_functions.ipynb:352-370) through the host-pointer entry.

        z: [T,N] (one panel shared by every run) or [B,T,N]; F0: [B,T,r] starting factors; r_each: [B] ints
        or None.  Returns dict(F [B,T,r], Lam [B,N,r], iters [B], ssr [B], ssr_path [B,path_cap] or None,
        R2 [B,N] or None)."""
        z = _NP.inp(z)
        F = _NP.upd(F0)
        B, T, r = F.shape
        if shared_panel is None:
            shared_panel = z.ndim == 2
        N = z.shape[-1]
        if z.shape[-2] != T or (not shared_panel and z.shape[0] != B):
            raise ValueError("z and F0 disagree on B or T")
        stride = 0 if shared_panel else T * N
        Lam = np.empty((B, N, r)); iters = np.empty(B, dtype=np.int32); ssr = np.empty(B)
        path = np.empty((B, path_cap)) if path_cap > 0 else None
        R2 = np.empty((B, N)) if want_R2 else None
        re = None if r_each is None else np.ascontiguousarray(r_each, dtype=np.int32)
        if re is not None and (re.shape != (B,) or re.min() < 1 or re.max() > r):
            raise ValueError("r_each must hold B values in 1..r")
        rc = self._lib.dfm_als_batch(self._h, B, T, N, r, _ptr(z), stride, _ptr(re), _ptr(F), _ptr(Lam), int(nt_min),
                                     int(min(max_iter, 2 ** 31 - 1)), float(tol), _ptr(path), int(path_cap), _ptr(iters),
                                     _ptr(ssr), _ptr(R2))
        _check(self._h, rc)
        return dict(F=F, Lam=Lam, iters=iters, ssr=ssr, ssr_path=path, R2=R2)

    def ols_batch_host(self, X, Y, nt_min: int = 0, shared_X: Optional[bool] = None, want_resid: bool = True):
        """Batched complete-case OLS (`ols_skipmissing`, dfm_functions.ipynb:242-252) through the host entry.

        X: [T,K] (shared regressors) or [P,T,K]; Y: [T,P] -- one problem per COLUMN (the reference's data
        layout) -- with NaN for missing.  Returns dict(beta [P,K], resid [T,P] or None, ssr, tss, nobs [P])."""
        X, Y = _NP.inp(X), _NP.inp(Y)
        T, P = Y.shape
        if shared_X is None:
            shared_X = X.ndim == 2
        K = X.shape[-1]
        if X.shape[-2] != T or (not shared_X and X.shape[0] != P):
            raise ValueError("X and Y disagree on T or P")
        beta = np.empty((P, K)); resid = np.empty((P, T)) if want_resid else None
        ssr = np.empty(P); tss = np.empty(P); nobs = np.empty(P, dtype=np.int32)
        rc = self._lib.dfm_ols_batch(self._h, P, T, K, _ptr(X), 0 if shared_X else T * K, _ptr(Y), 1, P, int(nt_min),
                                     _ptr(beta), _ptr(resid), _ptr(ssr), _ptr(tss), _ptr(nobs))
        _check(self._h, rc)
        return dict(beta=beta, resid=None if resid is None else resid.T.copy(), ssr=ssr, tss=tss, nobs=nobs)

    # ------------------------------------------------------------------ wild-bootstrap IRF bands (boot.hip)
    def var_bootstrap_irf_host(self, y, betahat, resid, p: int, H: int, ndraws: int, signs=None, seed: int = 0,
                               want_beta: bool = False, first_draw: int = 0):
        """B recursive-design wild-bootstrap draws of VAR(p) -> Cholesky -> impulse responses.
        y, resid: [T,ns] over the estimation window; betahat: [1 + ns p, ns].  Returns irf [B,ns,H,ns]
        (variable, horizon, shock) and, if asked, the re-estimated coefficients [B,1+ns p,ns]."""
        y, betahat = _NP.inp(y), _NP.inp(betahat)
        resid = _NP.inp(np.nan_to_num(resid))
        T, ns = y.shape
        B = int(ndraws)
        sg = None if signs is None else _NP.inp(signs)
        if sg is not None and sg.shape != (B, T):
            raise ValueError("signs must be [ndraws, T]")
        irf = np.empty((B, ns, H, ns)); bo = np.empty((B, 1 + ns * p, ns)) if want_beta else None
        rc = self._lib.dfm_var_bootstrap_irf(self._h, B, T, ns, int(p), int(H), _ptr(y), _ptr(betahat), _ptr(resid),
                                             _ptr(sg), ctypes.c_uint64(seed), ctypes.c_int64(first_draw), _ptr(bo), _ptr(irf))
        _check(self._h, rc)
        return (irf, bo) if want_beta else irf

    def quantile_bands_host(self, x, q):
        """Nearest-rank quantiles over the first axis: x [B, ...] -> [len(q), ...]."""
        x, q = _NP.inp(x), _NP.inp(q)
        B = x.shape[0]
        S = int(np.prod(x.shape[1:]))
        out = np.empty((q.size, S))
        rc = self._lib.dfm_quantile_bands(self._h, B, S, int(q.size), _ptr(x), _ptr(q), _ptr(out))
        _check(self._h, rc)
        return out.reshape((q.size,) + x.shape[1:])

    # ------------------------------------------------------------------ Chow / QLR with HAC covariance (breaks.hip)
    def chow_batch_host(self, ys, Xs, prob_series, prob_break, prob_q):
        """P Chow statistics with HAC covariance (`compute_chow`, dfm_functions.ipynb:891-902).  ys: list of S
        complete-case vectors, Xs: list of S matrices (T_s x k); problem p = (series, break date, bandwidth)."""
        S = len(ys)
        k = Xs[0].shape[1]
        Tlen = np.array([len(v) for v in ys], dtype=np.int32)
        Tmax = int(Tlen.max())
        y = np.zeros((S, Tmax)); X = np.zeros((S, Tmax, k))
        for s in range(S):
            y[s, :Tlen[s]] = ys[s]; X[s, :Tlen[s]] = Xs[s]
        ps, pb, pq = (np.ascontiguousarray(a, dtype=np.int32) for a in (prob_series, prob_break, prob_q))
        P = ps.size
        out = np.empty(P)
        rc = self._lib.dfm_chow_batch(self._h, S, Tmax, k, _ptr(y), _ptr(X), _ptr(Tlen), P, _ptr(ps), _ptr(pb), _ptr(pq),
                                      _ptr(out))
        _check(self._h, rc)
        return out

    def standardize_batch(self, panel, want_stats: bool = True):
        """`standardize_data` (dfm_functions.ipynb:501-509) of a device tensor [B,T,N] IN PLACE; returns (mean, sd)
        [B,N] device tensors (or None)."""
        be = _Torch(self, panel)
        B, T, N = panel.shape
        mu, sd = (be.out(B, N), be.out(B, N)) if want_stats else (None, None)
        be.sync()
        rc = self._lib.dfm_standardize_batch_dev(self._h, B, T, N, be.ptr(panel, "panel"), be.ptr(mu, "mean"), be.ptr(sd, "sd"))
        _check(self._h, rc)
        return mu, sd


from . import structural  # noqa: E402,F401  (attaches the structural entries to DfmContext)
from . import filtering  # noqa: E402,F401  (attaches the filter entries to DfmContext)
from . import gibbs  # noqa: E402,F401  (attaches the Gibbs sampler's entries to DfmContext)
from . import forecasting_ar  # noqa: E402,F401  (attaches the forecast entries of the AR-idiosyncratic model to DfmContext)
from . import filtering_ar  # noqa: E402,F401  (attaches its filter entries)
from . import simsmooth_ar  # noqa: E402,F401  (attaches its path-draw entries)
from . import gibbs_ar  # noqa: E402,F401  (attaches the Gibbs sampler's entries of the AR-idiosyncratic model)
from . import news_ar  # noqa: E402,F401  (attaches its news entries)
from . import simulate  # noqa: E402,F401  (attaches the simulated-panel entries of both models)
from . import rolling  # noqa: E402,F401  (attaches the rolling-window evaluation entries)
from . import diffusion  # noqa: E402,F401  (attaches the diffusion-index evaluation entries)
