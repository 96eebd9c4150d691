"""The two-way fixed-effects entry points without a GPU: the symbols are exported, sglm_fe2_plan's row lists,
chunks and components are right, the argument checks that touch no device refuse, and the model layer's
iterative dropping of uninformative levels equals a brute-force loop."""
import ctypes as C

import numpy as np
import pytest

import fe2_reference as F2
import fe_reference as FR
from sparkglm_amd import _lib as L

NEW = ("sglm_set_fe2", "sglm_fe2_plan", "sglm_fit_glm_fe2", "sglm_fe2_pass", "sglm_vcov_fe2", "sglm_get_fe2_ms")
T = 128


def test_symbols_are_exported_and_listed():
    lib = L.load()
    for s in NEW:
        assert hasattr(lib, s) and s in L.EXPORTS
    assert C.sizeof(L.Fe2Opts) == 16 and C.sizeof(L.Fe2Info) == 72  # sglm_fe2_opts, sglm_fe2_info
    assert lib.sglm_abi_version() == 8


@pytest.mark.parametrize("pat2", F2.PATTERNS2)
@pytest.mark.parametrize("pat1", ("sorted", "shuffled"))
def test_plan_lists_chunks_and_components(pat1, pat2):
    n = 2 * T + 1000 + 45
    ids1, G = FR.make_ids(pat1, n, T)
    ids2, H = F2.make_ids2(pat2, ids1, G)
    pl = L.fe2_plan(ids1, ids2, G, H)
    clen, start, level, rows = pl["chunk_len"], pl["chunk_start"], pl["chunk_level"], pl["list"]
    assert clen >= 32 and clen % 32 == 0
    # the chunks cover the list once, in order, each within one level and at most chunk_len long
    assert start[0] == 0 and start[-1] == n and np.all(np.diff(start) > 0) and np.all(np.diff(start) <= clen)
    assert sorted(rows.tolist()) == list(range(n))
    assert np.all(np.diff(level) >= 0)  # ordered by level: the combine tree reads them as they lie
    for k in range(len(level)):
        r = rows[start[k]:start[k + 1]]
        assert np.all(ids2[r] == level[k]) and np.all(np.diff(r) > 0)  # ascending rows within a level
    counts = np.bincount(ids2, minlength=H)
    assert len(level) == int(np.sum((counts + clen - 1) // clen)) <= H + (n + clen - 1) // clen
    for h in range(H):  # a level's rows ascend across its chunks too
        assert np.array_equal(rows[np.isin(rows, np.flatnonzero(ids2 == h))], np.flatnonzero(ids2 == h))
    _, _, low = F2.components(ids1, ids2, G, H)
    assert pl["ncomp"] == len(low) and np.array_equal(pl["comp_low"], low)
    want = dict(cycle=1, random=1, two_comp=2, nested=4, giant=1, empty=1, single=1)[pat2]
    assert pl["ncomp"] == want


def test_plan_refuses_codes_out_of_range():
    ids1, ids2 = np.array([0, 1, 2, 1]), np.array([0, 1, 0, 1])
    assert L.fe2_plan(ids1, ids2, 3, 2)["ncomp"] == 2  # {0, 2 | 0} and {1 | 1}
    for a, b, G, H in ((ids1, ids2, 2, 2), (ids1, ids2, 3, 1), (ids1 - 1, ids2, 3, 2), (ids1, ids2 - 1, 3, 2)):
        with pytest.raises(L.IllegalArgumentException, match="every code"):
            L.fe2_plan(a, b, G, H)
    with pytest.raises(L.IllegalArgumentException, match="same number of rows"):
        L.fe2_plan(ids1, ids2[:-1], 3, 2)
    empty = L.fe2_plan(np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), 2, 2)
    assert empty["ncomp"] == 0 and len(empty["chunk_level"]) == 0


def test_refusals_that_touch_no_device():
    lib = L.load()
    o = L.GlmOpts(2, 4, 1e-6, 0, 0, 0, 0)  # poisson / log
    bad = L.GlmOpts(2, 0, 1e-6, 0, 0, 0, 0)  # poisson / logit
    fo = L.Fe2Opts(0.0, 0)
    p = 3
    coefs, se, alpha, gamma = np.zeros(p), np.zeros(p), np.zeros(4), np.zeros(2)
    cov = np.zeros((p, p), order="F")
    pre = L.PreGLM(L.ptr(coefs), L.ptr(se), 0, 0, 0, 0, 0, 0, 0, None, 0)
    info = L.Fe2Info()
    E = L.SGLM_EINVAL
    fit = lib.sglm_fit_glm_fe2
    assert fit(None, C.byref(o), C.byref(fo), C.byref(pre), L.ptr(alpha), L.ptr(gamma), C.byref(info)) == E
    assert "null engine handle" in L.last_error()
    assert fit(None, C.byref(o), None, None, L.ptr(alpha), L.ptr(gamma), None) == E
    assert fit(None, C.byref(o), None, C.byref(pre), L.ptr(alpha), None, None) == E
    assert "gamma" in L.last_error()
    assert fit(None, C.byref(bad), None, C.byref(pre), L.ptr(alpha), L.ptr(gamma), None) == E
    assert "family/link" in L.last_error()
    assert fit(None, None, None, C.byref(pre), L.ptr(alpha), L.ptr(gamma), None) == E
    assert lib.sglm_fe2_pass(None, C.byref(o), None, None, None, None, None, None, None, None, None, None, None) == E
    assert lib.sglm_vcov_fe2(None, C.byref(o), None, L.ptr(coefs), L.ptr(alpha), L.ptr(gamma), 1, 1, 1,
                             cov.ctypes.data_as(L.dp), None) == E
    assert lib.sglm_vcov_fe2(None, C.byref(o), None, L.ptr(coefs), L.ptr(alpha), None, 0, 0, 0,
                             cov.ctypes.data_as(L.dp), None) == E
    for hc in (2, 3):  # HC2 / HC3 under clustering, before the handle is looked at
        assert lib.sglm_vcov_fe2(None, C.byref(o), None, L.ptr(coefs), L.ptr(alpha), L.ptr(gamma), 1, hc, 1,
                                 cov.ctypes.data_as(L.dp), None) == E
        assert "HC2 / HC3" in L.last_error()
    assert lib.sglm_set_fe2(None, None, 0, 0) == E
    assert lib.sglm_get_fe2_ms(None, L.ptr(np.zeros(5))) == E


def test_iterative_dropping_equals_the_brute_force_loop():
    """Dropping a unit's rows can leave a period without information: the model layer's vectorised loop
    (glm.fe2_drop) against the brute-force one.  Binomial, m = 6, built so that three rounds are needed: unit 3 is
    all 0; period 7 is all m except in unit 3's rows, so it goes once they are gone; unit 5 is all 0 except in
    period 7, so it goes after that.  (With counts one round always suffices: the dropped rows are all zero.)"""
    from sparkglm_amd.glm import fe2_drop
    rng = np.random.default_rng(5)
    n = 600
    ids1, ids2 = rng.integers(0, 30, n), rng.integers(0, 12, n)
    m = np.full(n, 6.0)
    y = rng.integers(1, 6, n).astype(np.float64)
    ids2[np.flatnonzero(ids1 == 3)[:2]] = 7
    ids2[np.flatnonzero(ids1 == 5)[:2]] = 7
    y[ids1 == 5] = 0.0
    y[ids2 == 7] = 6.0
    y[ids1 == 3] = 0.0
    prior = np.ones(n)
    free = np.flatnonzero((ids1 != 3) & (ids1 != 5) & (ids2 != 7))
    prior[rng.choice(free, 40, replace=False)] = 0.0
    keep, rounds = fe2_drop(ids1, ids2, y, "binomial", m, prior)
    want, wrounds = F2.drop_uninformative(ids1, ids2, y, "binomial", m, prior)
    assert np.array_equal(keep, want) and rounds == wrounds == 3
    assert not keep[(ids1 == 3) | (ids1 == 5) | (ids2 == 7)].any() and keep.sum() == np.sum((ids1 != 3) & (ids1 != 5) & (ids2 != 7))
    # counts: unit 3 all zero and period 7 zero outside it -- one round; gaussian: nothing is uninformative
    yc = rng.poisson(1.5, n).astype(np.float64) + 1.0
    yc[(ids1 == 3) | (ids2 == 7)] = 0.0
    keep, rounds = fe2_drop(ids1, ids2, yc, "poisson", None, prior)
    want, wrounds = F2.drop_uninformative(ids1, ids2, yc, "poisson", None, prior)
    assert np.array_equal(keep, want) and rounds == wrounds == 1 and not keep[(ids1 == 3) | (ids2 == 7)].any()
    keep, rounds = fe2_drop(ids1, ids2, yc, "gaussian", None, prior)
    assert keep.all() and rounds == 0
