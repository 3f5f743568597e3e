"""epnp::gauss_newton with one column of the 6 x 4 system per lane (gauss_newton of csrc/svo_epnp_ord_dev.h), the part that needs no
GPU: the fixture tests/golden/epnp_gn_cases.npy (tools/make_epnp_gn_cases.py) holds the branches of qr_solve it was made for, and
the ordering argument - a Householder step's column updates are independent, `b <- Q^T b` is one more column - holds bit for bit:
a C restatement of the lanes' walk (shim_gn_cols of tools/epnp_gn_shim.c) against the CPU restatement's gauss_newton itself."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_epnp_gn_cases as mk             # noqa: E402


@pytest.fixture(scope="module")
def cases():
    return np.load(mk.PATH)


@pytest.fixture(scope="module")
def lib():
    return mk.shim()


def same_bits(a, b):
    """Equal as uint64 wherever not both are NaN (payloads are not compared), and NaN in the same places."""
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb])


def test_fixture_holds_the_branches_it_was_made_for(cases):
    """Per Householder step k: at least 10 systems with a negative pivot and 10 with eta taken from below the diagonal; eta == 0 at
    k = 0 (all betas zero) and k = 3 (columns 6..9 of L zero), each also in one candidate only, and at k = 0 in a later iteration
    only; candidates of shape 2 and 3; at least 20 calls whose candidates part ways in a step (sign of the pivot, eta == 0); at least
    5 systems whose pivot column's largest entry, by 1e6, sits in the row the scan never looks at; an infinity and a NaN in L."""
    assert cases.dtype == mk.CASE and len(cases) <= 400
    figures = mk.coverage(cases)
    print(figures)
    assert set(cases["kind"].tolist()) == set(mk.KINDS)


def test_recorded_results_are_the_restatements(cases, lib):
    for i, c in enumerate(cases):
        for k in range(3):
            assert same_bits(mk.walk(lib, c["L"], c["rho"], c["bin"][k]), c["bout"][k]), (i, k)


def test_column_ordered_walk_equals_gauss_newton_on_the_fixture(cases, lib):
    for i, c in enumerate(cases):
        for k in range(3):
            got = mk.walk(lib, c["L"], c["rho"], c["bin"][k], "shim_gn_cols")
            assert same_bits(got, c["bout"][k]), (i, k, int(c["kind"]), got, c["bout"][k])


def test_column_ordered_walk_equals_gauss_newton_on_100000_seeded_systems(lib):
    """Random L, rho and start values in the three candidate shapes, a third of them with L scaled by 1e-3 and a third with
    small-integer L (exact zeros and ties in the eta scan)."""
    n = 100000
    rng = np.random.default_rng(7)
    L = rng.normal(size=(n, 60))
    L[1::3] *= 1e-3
    L[2::3] = rng.integers(-3, 4, size=L[2::3].shape)
    rho = rng.normal(size=(n, 6))
    b = rng.normal(size=(n, 4))
    b[1::4, 2:] = 0.0
    b[2::4, 3] = 0.0
    b[3::400] = 0.0
    ref, got = b.copy(), b.copy()
    lib.shim_gn_many(0, n, mk._p(L), mk._p(rho), mk._p(ref))
    lib.shim_gn_many(1, n, mk._p(L), mk._p(rho), mk._p(got))
    na, nb = np.isnan(ref), np.isnan(got)
    assert np.array_equal(na, nb)
    bad = np.flatnonzero(((ref.view(np.uint64) != got.view(np.uint64)) & ~na).any(axis=1))
    assert bad.size == 0, (bad[:8], ref[bad[:1]], got[bad[:1]])
    assert not np.array_equal(ref, b)
