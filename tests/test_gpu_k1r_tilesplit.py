"""K1r's tile map at 16 column blocks (p = 225..256; fused.hpp TilesR<16, WV>, SGLM_K1R_ISPLIT): which
Gram wave owns which of the 136 tiles of X'WX is a compile-time table, and Gram waves 0..3 -- the ones
that also issue the LDS-DMA -- may hold fewer tiles than their SIMD partners 4..7.  Whatever the table,
every tile sums the same k-steps in the same order, so K1r stays BITWISE K1 (SGLM_FUSED_SPLIT=0).  The
same holds for the issue priority the two Gram waves of a SIMD run their k-steps at (SGLM_K1R_IPRIO): it
moves when a wave reaches a hand-off, never what it sums.

  * K1 against K1r, each in a fresh child process (this file run as a script, the kernel chosen by the
    environment the child starts with), on p = 256, 241 and 225 and rows 1, 31, 33, 64, 97 (zero to three
    full blocks and a ragged last one in the first workgroup), 32 * grid + 5 (one block per workgroup, a few
    with two) and 40 * 32 * grid + 7 (about 40 blocks per workgroup: the ring's counters advance many
    rounds while the waves that own more tiles fall behind the ones that own fewer): binomial / logit with
    and without offset + prior weights, and gamma / inverse, whose row stage defers nothing.  Pass outputs
    at beta and of the initial pass; where a fit has enough rows, its coefficients, standard errors,
    scalars and deviance trace.
  * A design whose Gram is known exactly: column block b holds +-2^e(b) (1 + c / 16), c the column within
    the block, the exponents a Sidon set -- every pair of blocks has its own power of two, so a tile that
    no wave owns (zeros), or that a wave stores under another tile's index, shows in that tile.  Gaussian /
    identity at beta = 0 (w = 1, z = y): every product and sum is exact in binary64.  Every tile of X'X and
    every block of X'y is checked on its own, to 1e-12 relative.
  * A fit's deviance-only passes (no Gram: the Gram waves only hand the ring on) against the same fit
    with SGLM_SPECULATE=0, bitwise, at p = 256."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (256, 241, 225)
SMALL_ROWS = (1, 31, 33, 64, 97)
RB = 32  # rows of a block


def _rows(grid):
    return SMALL_ROWS + (RB * grid + 5,)


def _logit_case(n, p, weights):
    """Host data: the design in column-major order without a transposing copy."""
    rng = np.random.default_rng(100_003 * p + n + (7 if weights else 0))
    X = (rng.random((p, n)) * 2.0 - 1.0).T
    X[:, 0] = 1.0
    beta = rng.normal(0.0, 0.05, p)
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-(X @ beta)))).astype(np.float64)
    kw = {}
    if weights:
        kw = dict(offset=rng.uniform(-0.2, 0.2, n), prior=rng.uniform(0.5, 2.0, n))
        kw["prior"][rng.random(n) < 0.05] = 0.0
    return X, y, beta, kw


def _fit_arrays(f):
    return {"fit": np.concatenate([np.ravel(f.coefs), np.ravel(f.stderr),
                                   [f.deviance, f.null_deviance, f.pearson, f.loglik, float(f.iter)]]),
            "dev_trace": np.asarray(f.dev_trace, dtype=np.float64)}


def child(out_path):
    """Every case under the kernel SGLM_FUSED_SPLIT selects; the results as arrays in out_path."""
    sys.path.insert(0, ROOT)
    from sparkglm_amd import Engine

    res = {}
    kernels = set()

    def passes(e, key, beta, family, link, mu0, fit):
        for tag, r in (("pass", e.irls_pass(beta, family=family, link=link)),
                       ("init", e.irls_pass(None, mu0=mu0, family=family, link=link))):
            for name, a in zip(("gram", "xz", "scalars"), r):
                res[f"{key}:{tag}:{name}"] = np.ascontiguousarray(a)
        if fit:
            for name, a in _fit_arrays(e.fit_glm(family, link)).items():
                res[f"{key}:{name}"] = a
        kernels.add(e.stats()["pass_kernel"])

    with Engine(0) as e:
        e.synth(0, 0, 100_000, 256, 1)  # more blocks than workgroups: the pass runs its full grid
        e.irls_pass(np.zeros(256))
        grid = int(e.stats()["workgroups"])
        res["grid"] = np.array([grid], dtype=np.float64)
        for p in WIDTHS:
            for n in _rows(grid):
                for weights in (False, True):
                    X, y, beta, kw = _logit_case(n, p, weights)
                    e.set_data(X, y, **kw)
                    passes(e, f"logit:{p}:{n}:{int(weights)}", beta, "binomial", "logit", 0.3, n > 2 * p)
        # gamma / inverse (the device generator's positive design): the row stage without the deferred deviance
        for p, n in ((256, 97), (241, RB * grid + 5)):
            rng = np.random.default_rng(p)
            beta = np.abs(rng.normal(0.0, 0.02, p)) + 0.01
            beta[0] = 1.0
            e.synth(3, 0, n, p, 11)
            passes(e, f"gamma:{p}:{n}", beta, "gamma", "inverse", 1.3, False)
        # about 40 blocks per workgroup
        n = 40 * RB * grid + 7
        e.synth(0, 0, n, 256, 11)
        passes(e, "logit:256:long:0", np.random.default_rng(5).normal(0.0, 0.02, 256), "binomial", "logit", 0.3, True)
        X, y, beta, kw = _logit_case(n, 241, True)
        e.set_data(X, y, **kw)
        passes(e, "logit:241:long:1", beta, "binomial", "logit", 0.3, True)
    res["kernels"] = np.array(sorted(kernels), dtype=np.float64)
    np.savez(out_path, **res)


@pytest.fixture(scope="module")
def k1_and_k1r(tmp_path_factory):
    """(K1's arrays, K1r's arrays), each computed once by a child process of its own."""
    out = []
    for split in ("0", "1"):
        path = str(tmp_path_factory.mktemp("tilesplit") / f"split{split}.npz")
        env = dict(os.environ, SGLM_FUSED_SPLIT=split)
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], env=env, check=True, timeout=600)
        with np.load(path) as z:
            out.append({k: z[k] for k in z.files})
    return out


def test_children_ran_k1_and_k1r(k1_and_k1r):
    k1, k1r = k1_and_k1r
    assert k1["kernels"].tolist() == [1.0] and k1r["kernels"].tolist() == [2.0]  # sglm.h sglm_pass_kernel
    assert set(k1) == set(k1r) and k1["grid"][0] == k1r["grid"][0] >= 1


def _assert_bitwise(k1, k1r, prefix, need):
    keys = sorted(k for k in k1 if k.startswith(prefix))
    assert {k[len(prefix):] for k in keys} >= set(need), (prefix, keys)
    for k in keys:
        a, b = k1[k], k1r[k]
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), k  # bit for bit, NaNs included


PASS_KEYS = [f"{t}:{a}" for t in ("pass", "init") for a in ("gram", "xz", "scalars")]
FIT_KEYS = ["fit", "dev_trace"]


@pytest.mark.parametrize("weights", [0, 1], ids=["plain", "offset+prior"])
@pytest.mark.parametrize("rows", list(SMALL_ROWS) + ["grid"])
@pytest.mark.parametrize("p", WIDTHS)
def test_logit_bitwise_k1(k1_and_k1r, p, rows, weights):
    k1, k1r = k1_and_k1r
    n = RB * int(k1["grid"][0]) + 5 if rows == "grid" else rows
    _assert_bitwise(k1, k1r, f"logit:{p}:{n}:{weights}:", PASS_KEYS + (FIT_KEYS if n > 2 * p else []))


@pytest.mark.parametrize("case", ["logit:256:long:0", "logit:241:long:1"])
def test_forty_blocks_per_workgroup_bitwise_k1(k1_and_k1r, case):
    k1, k1r = k1_and_k1r
    _assert_bitwise(k1, k1r, case + ":", PASS_KEYS + FIT_KEYS)


def test_gamma_inverse_bitwise_k1(k1_and_k1r):
    k1, k1r = k1_and_k1r
    n = RB * int(k1["grid"][0]) + 5
    _assert_bitwise(k1, k1r, "gamma:256:97:", PASS_KEYS)
    _assert_bitwise(k1, k1r, f"gamma:241:{n}:", PASS_KEYS)


# Mian-Chowla: every sum of two terms (a term with itself included) is distinct
SIDON = (1, 2, 4, 8, 13, 21, 31, 45, 66, 81, 97, 123, 148, 182, 204, 252)


def _engine(var, value):
    from sparkglm_amd import Engine
    saved = os.environ.get(var)
    os.environ[var] = value
    try:
        return Engine(0)
    finally:
        if saved is None:
            os.environ.pop(var, None)
        else:
            os.environ[var] = saved


@pytest.mark.parametrize("n", [97, 9_477])  # three ragged blocks; 296 blocks and 5 rows
@pytest.mark.parametrize("p", [256, 241])
def test_every_tile_against_the_closed_form(p, n):
    sums = [a + b for i, a in enumerate(SIDON) for b in SIDON[: i + 1]]
    assert len(set(sums)) == len(sums) == 136
    rng = np.random.default_rng(n + p)
    col = np.arange(p)
    scale = np.ldexp(1.0 + (col % 16) / 16.0, np.asarray(SIDON)[col // 16] - 126)  # 2^e(b) (1 + c / 16)
    sign = rng.choice([-1.0, 1.0], n)
    y = rng.integers(-8, 9, n).astype(np.float64)
    X = np.asfortranarray(sign[:, None] * scale[None, :])
    gram_ref = float(n) * np.outer(scale, scale)  # exact: sign^2 = 1, 8-bit significands, n < 2^53
    xz_ref = scale * float(np.dot(sign, y))       # exact: an integer times the column's scale
    with _engine("SGLM_FUSED_SPLIT", "1") as e:
        e.set_data(X, y)
        g, xz, _ = e.irls_pass(np.zeros(p), family="gaussian", link="identity")
        assert e.stats()["pass_kernel"] == 2  # K1r (sglm.h sglm_pass_kernel)
    nb = (p + 15) // 16
    bad = []
    for bi in range(nb):
        r = slice(16 * bi, min(16 * bi + 16, p))
        if np.max(np.abs(xz[r] - xz_ref[r]) / np.maximum(np.abs(xz_ref[r]), 1e-300)) > 1e-12:
            bad.append(("X'Wz", bi))
        for bj in range(bi + 1):
            c = slice(16 * bj, min(16 * bj + 16, p))
            for blk, ref, name in ((g[r, c], gram_ref[r, c], "lower"), (g[c, r].T, gram_ref[r, c], "upper")):
                if np.max(np.abs(blk - ref) / np.abs(ref)) > 1e-12:
                    bad.append((name, bi, bj))
    assert not bad, bad


def test_deviance_only_pass_bitwise_the_full_pass():
    n, p = 24_589, 256
    fits = []
    for spec in ("1", "0"):
        with _engine("SGLM_SPECULATE", spec) as e:
            e.synth(0, 0, n, p, 11)
            e.reset_stats()
            f = e.fit_glm("binomial", "logit")
            st = e.stats()
            assert st["pass_kernel"] == 2
            fits.append((_fit_arrays(f), st["dev_passes"]))
    (a, da), (b, db) = fits
    assert da >= 1 and db == 0
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        child(sys.argv[2])
