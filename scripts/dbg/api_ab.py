#!/usr/bin/env python
"""api.py under TWO trees, from identical inputs and without a device: the call list and the refusal table of tests/api_calls.py
run once under each tree's dynamic_factor_models_amd (one process per tree, each dumping its records), then compared bit for bit.
The binding is this tree's stand-in (tests/api_calls.py) in both runs; only the package differs.  For host refactors of api.py.
Usage: python scripts/dbg/api_ab.py parent=<path of a checkout of the parent commit> [out=<file>]
  Per call of the list, in four runs (as listed; the first library call failing with -5; the same with the Gibbs sampler's message;
  without ctx, so that api._own makes the context) and, where it makes several library calls, a fifth with the last one failing
  (estimate()'s EM behind its start; a band call behind a retried one): every recorded argument of every binding call (arrays by shape, dtype and
  bytes, NaN positions included; scalars and keyword arguments by type and value), the library calls by name and integers, every
  leaf of the returned value or the exception's type and text, how often the context was closed, and the model before and after.
  Per refusal: the exception's type and text.  And api's public names with their signatures and docstrings.  Both runs are the
  same NumPy on the same machine, so there is no tolerance: exit status 1 on any difference.
       python scripts/dbg/api_ab.py mode=record out=tests/golden/api_calls.json
  The structure that tests/test_api_calls_cpu.py holds this tree to (binding calls as text, returned keys and shapes), from THIS
  tree.  A change of that file is a change of behaviour: it belongs in the diff of the change that means it, never in a refactor."""
import importlib.util, inspect, json, os, pickle, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ARGS = dict(a.split("=", 1) for a in sys.argv[1:])
MODE = ARGS.get("mode", "ab")
OUT = open(ARGS["out"], "w") if "out" in ARGS and MODE == "ab" else None
GIBBS_TEXT = "Gibbs sampler: the Cholesky factor of a regression's precision does not exist"


def say(s=""):
    print(s, flush=True)
    if OUT: OUT.write(s + "\n"); OUT.flush()


def load_calls(root):
    """tests/api_calls.py of THIS tree on top of the package of tree `root`."""
    sys.path.insert(0, os.path.abspath(root))
    spec = importlib.util.spec_from_file_location("api_calls_ab", os.path.join(ROOT, "tests", "api_calls.py"))
    ac = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ac)
    assert os.path.samefile(os.path.dirname(os.path.dirname(ac.api.__file__)), root), ac.api.__file__
    return ac


def plain(rec):
    err = None if rec.error is None else (type(rec.error).__name__, str(rec.error))
    return dict(log=rec.log, lib=rec.lib, result=rec.result, error=err, closed=rec.closed, before=rec.model_before,
                after=rec.model_after)


def mode_dump():
    """(a child of mode_ab) every record of tree root=, pickled to out="""
    import warnings
    warnings.simplefilter("ignore")                      # the fills are no estimates: logs and divisions complain, equally in both trees
    ac = load_calls(ARGS["root"])
    runs = {}
    for c in ac.CALLS:
        runs[c.id] = plain(ac.run(c))
        runs[c.id + " | -5"] = plain(ac.run(c, fail=(1, -5, "not positive definite")))
        runs[c.id + " | -5, Gibbs"] = plain(ac.run(c, fail=(1, -5, GIBBS_TEXT)))
        runs[c.id + " | own context"] = plain(ac.run(c, own=True))
        last = sum(n != "dfm_last_error" for n, _ in runs[c.id]["lib"])
        if last > 1:
            runs[c.id + " | -5 at the last call"] = plain(ac.run(c, fail=(last, -5, "not positive definite")))
    refusals = {}
    for i, r in enumerate(ac.REFUSALS):
        e = ac.refuse(r)
        refusals[f"{r.fn} #{i}: {r.wins}"] = (type(e).__name__, str(e))
    public = {}
    for n in sorted(n for n in dir(ac.api) if not n.startswith("_")):
        v = getattr(ac.api, n)
        if inspect.ismodule(v): public[n] = "module"
        elif getattr(v, "__module__", ac.api.__name__) != ac.api.__name__: public[n] = "from " + v.__module__
        elif callable(v): public[n] = (str(inspect.signature(v)) if not inspect.isclass(v) or v.__init__ is not object.__init__ else "()", inspect.getdoc(v))
        else: public[n] = repr(v)
    with open(ARGS["out"], "wb") as f:
        pickle.dump(dict(runs=runs, refusals=refusals, public=public), f)
    return 0


def differences(a, b, where=""):
    """Where two records differ, as texts; [] when they are equal bit for bit."""
    import numpy as np
    if type(a) is not type(b):
        return [f"{where}: {type(a).__name__} against {type(b).__name__}"]
    if isinstance(a, np.ndarray):
        if a.shape != b.shape or a.dtype != b.dtype:
            return [f"{where}: {a.dtype}{list(a.shape)} against {b.dtype}{list(b.shape)}"]
        return [] if np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes() else [f"{where}: the bytes differ"]
    if isinstance(a, dict):
        if list(a) != list(b):
            return [f"{where}: keys {list(a)} against {list(b)}"]
        return [d for k in a for d in differences(a[k], b[k], f"{where}[{k!r}]")]
    if isinstance(a, (list, tuple)):
        if len(a) != len(b):
            return [f"{where}: {len(a)} items against {len(b)}"]
        return [d for i, (x, y) in enumerate(zip(a, b)) for d in differences(x, y, f"{where}[{i}]")]
    if isinstance(a, (float, np.floating)):
        return [] if np.float64(a).tobytes() == np.float64(b).tobytes() else [f"{where}: {a!r} against {b!r}"]
    return [] if a == b else [f"{where}: {a!r} against {b!r}"]


def mode_ab():
    parent = os.path.abspath(ARGS["parent"])
    got = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, root in (("parent", parent), ("new", ROOT)):
            out = os.path.join(tmp, name + ".pkl")
            subprocess.run([sys.executable, os.path.abspath(__file__), "mode=dump", "root=" + root, "out=" + out], check=True,
                           cwd=tmp, env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"))
            with open(out, "rb") as f:
                got[name] = pickle.load(f)
    say("api.py: the new tree against the parent, every binding argument, returned leaf, exception and model field bit for bit")
    bad = 0
    for part in ("public", "refusals", "runs"):
        p, n = got["parent"][part], got["new"][part]
        if list(p) != list(n):
            bad += 1
            say(f"{part}: the entries differ: only the parent has {sorted(set(p) - set(n))}, only the new tree {sorted(set(n) - set(p))}")
        for k in p:
            if k not in n: continue
            d = differences(p[k], n[k], k)
            bad += bool(d)
            if part == "runs":
                r = p[k]
                what = f"{len(r['log'])} binding call(s), " + (f"{r['error'][0]}" if r["error"] else "returned") + f", closed {r['closed']}x"
                say(f"{k:<60}{what:<46}{'equal' if not d else 'DIFFERS'}")
            elif part == "refusals":
                say(f"{k:<106}{'equal' if not d else 'DIFFERS'}")
            for line in d[:8]: say("    " + line)
        if part == "public":
            say(f"public names ({len(p)}), signatures and docstrings: {'equal' if not bad else 'DIFFER'}")
    n_runs, n_ref = len(got["parent"]["runs"]), len(got["parent"]["refusals"])
    say(f"{bad} entr(ies) differ" if bad else f"all {n_runs} runs and {n_ref} refusals equal bit for bit; public names, signatures and docstrings equal")
    return 1 if bad else 0


def mode_record():
    import warnings
    warnings.simplefilter("ignore")
    ac = load_calls(ROOT)
    table = {}
    for c in ac.CALLS:
        r = ac.run(c)
        assert r.error is None, (c.id, r.error)
        table[c.id] = dict(calls=[ac.call_text(e) for e in r.log], result=ac.result_text(r.result))
    with open(ARGS["out"], "w") as f:
        json.dump(table, f, indent=1)
        f.write("\n")
    print(f"{len(table)} calls recorded in {ARGS['out']}")
    return 0


sys.exit(dict(ab=mode_ab, dump=mode_dump, record=mode_record)[MODE]())
