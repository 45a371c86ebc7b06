"""What tests/test_gpu_coarse.py and tests/test_gpu_coarse_shapes.py share: one run of an engine over a set of genomes with
KR_OPT_COARSE_REST on or off, and the rule of both files -- candidates (prefix, in_mask, out_mask) in order, records in the order
kr_fetch returns them, count(g) and -- where asked -- keys(g) are BIT-IDENTICAL between the option's two settings and equal
to oracle/kmer_oracle.c."""
import numpy as np

_REF = {}


def _reference(K, name, texts, flags, ldr, omit=False, apply_filter=True):
    """the oracle's answer, once per named input"""
    if name not in _REF:
        L, Dg, R = ldr
        keys = [K.sorted_keys(t.tobytes(), L, Dg, R, omit=omit) for t in texts]
        cands = K.intersect(keys, flags, L, Dg, R, apply_filter=apply_filter)
        recs = np.sort(K.collect(keys, cands, L, Dg, R), order=["key", "genome"])
        for a in keys + [cands, recs]:
            a.setflags(write=False)
        _REF[name] = (keys, cands, recs)
    return _REF[name]


def _run(N, texts, flags, ldr, coarse_rest, coarse_ids=None, step=None, lanes=None, omit=False, apply_filter=True,
         keys_of=(), steps=1):
    """one engine: upload, then either `step` (distributed.sharded_step) `steps` times or sort / partition (`coarse_ids`) +
    intersect + collect by hand -> dict of everything compared"""
    out = {}
    ids = list(range(len(texts)))
    with N.Engine() as e:
        e.set_option(N.OPT_COARSE_REST, coarse_rest)
        if lanes is not None:
            e.set_option(N.OPT_LANES, lanes)
        e.set_params(*ldr, omit_soft=omit, max_bases=max(len(t) for t in texts))
        for g, t in zip(ids, texts):
            e.upload(g, t)
        assert e.debug_info()["b"] > 8
        for _ in range(steps):
            if step is not None:
                n, nrec = step(e, ids, flags, 1, apply_filter=apply_filter)
                recs = e.fetch_records(nrec)
            else:
                for g in ids:
                    (e.partition if g in coarse_ids else e.sort)(g)
                n = e.intersect(ids, flags, apply_filter=apply_filter)
                recs = e.collect(ids)
            out.setdefault("cands", []).append(e.cands().copy())
            out.setdefault("recs", []).append(recs.copy())
            assert n == len(out["cands"][-1])
        out["lazy_before_counts"] = e.debug_lazy()
        out["counts"] = [e.count(g) for g in ids]
        out["lazy"] = e.debug_lazy()                 # (counting promotes nothing)
        assert out["lazy"]["coarse_promoted"] == out["lazy_before_counts"]["coarse_promoted"]
        out["keys"] = {g: e.keys(g) for g in keys_of}
        out["lazy_after_keys"] = e.debug_lazy()
    return out


def _same(a, b):
    assert len(a["cands"]) == len(b["cands"])
    for x, y in zip(a["cands"], b["cands"]):
        assert np.array_equal(x, y), "candidates differ between KR_OPT_COARSE_REST = 1 and 0"
    for x, y in zip(a["recs"], b["recs"]):
        assert np.array_equal(x, y), "records (in kr_fetch order) differ between KR_OPT_COARSE_REST = 1 and 0"
    assert a["counts"] == b["counts"]
    for g in a["keys"]:
        assert np.array_equal(a["keys"][g], b["keys"][g])


def _oracle(out, ref):
    keys, cands, recs = ref
    for c in out["cands"]:
        assert len(c) == len(cands)
        for f in ("prefix", "in_mask", "out_mask"):
            assert np.array_equal(c[f], cands[f]), f
    for r in out["recs"]:
        assert np.array_equal(np.sort(r, order=["key", "genome"]), recs)
    assert out["counts"] == [len(k) for k in keys]
    for g, k in out["keys"].items():
        assert np.array_equal(k, keys[g]), f"sorted keys of genome {g}"


def _ab(N, K, name, texts, flags, ldr=(25, 1, 2), coarse_expected=None, promoted_expected=None, **kw):
    """both settings of the option against each other and against the oracle; -> the run with the option on"""
    on = _run(N, texts, flags, ldr, 1, **kw)
    off = _run(N, texts, flags, ldr, 0, **kw)
    assert off["lazy"]["coarse"] == 0 and off["lazy_after_keys"]["coarse_promoted"] == 0
    _same(on, off)
    _oracle(on, _reference(K, name, texts, flags, ldr, omit=kw.get("omit", False), apply_filter=kw.get("apply_filter", True)))
    if coarse_expected is not None:
        assert on["lazy"]["coarse"] == coarse_expected, on["lazy"]
    if promoted_expected is not None:
        assert on["lazy"]["coarse_promoted"] == promoted_expected, on["lazy"]
    return on
