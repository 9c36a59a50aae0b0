"""CPU: the control logic of the block-Lanczos eigen-solver
(minimization/block_lanczos.py) and of the ELBO's batching, with a numpy pair
of `dots` / `axpy` passed in as a test double (the package itself supplies the
native pair only).  The kernels are tested on the GPU in
test_eig_kernels_gpu.py."""
import numpy as np
import pytest

from conftest import golden

from nifty_amd.evidence_lower_bound import batch_sizes, elbo_statistics, metric_spectrum, shared_spectrum
from nifty_amd.minimization.block_lanczos import largest_eigenpairs


class NumpyOps:
    kmax = 8

    def zeros(self, rows, n):
        return np.zeros((rows, n))

    def set(self, rows, host):
        rows[:] = host

    def dots(self, V, W):
        return V @ W.T

    def axpy(self, V, T, W, beta):
        W[:] = (W if beta else 0.0) + T.T @ V


def matvec_of(A):
    count = [0]

    def mv(X, Y):
        assert X.shape == Y.shape and 1 <= X.shape[0] <= 8
        count[0] += X.shape[0]
        Y[:] = X @ A

    mv.count = count
    return mv


def spd(n, seed, decay=0.8):
    """a dense symmetric positive definite matrix with the spectrum
    10 * decay^i and its eigen-decomposition (descending)"""
    rng = np.random.default_rng(seed)
    U = np.linalg.qr(rng.standard_normal((n, n)))[0]
    lam = 10.0 * decay ** np.arange(n)
    return (U * lam) @ U.T, lam, U


# golden fixture tolerance of "Tolerance for (b), (c) and (d)": 10 x the larger
# of a fixture's two discrepancies, relative to lambda_max.  A synthetic matrix
# belongs to none of the three fixtures, so it gets the tightest of them.
def fixture_tol():
    G = golden("elbo.npz")
    return min(float(G[f"{k}_tol"]) for k in ("a", "c", "d"))


def test_diagonal_degenerate_top_refills():
    """triple-degenerate top eigenvalue, block 2 < multiplicity, nev = 5 no
    multiple of the block: the Krylov space of a block of 2 holds two copies
    only, so the third comes from the refill path"""
    lam = np.zeros(40)
    lam[:7] = [10, 10, 10, 7, 5, 3, 2]
    res = largest_eigenpairs(matvec_of(np.diag(lam)), NumpyOps(), 40, 5, rng=np.random.default_rng(1), block=2)
    assert res.refills > 0
    np.testing.assert_allclose(res.values, [10, 10, 10, 7, 5], rtol=0, atol=1e-13)
    V = np.asarray(res.vectors)
    assert np.abs(V @ V.T - np.eye(5)).max() < 1e-12
    assert np.abs(V @ np.diag(lam) - res.values[:, None] * V).max() < 1e-12


def test_diagonal_degenerate_top_block8():
    """the same spectrum with the default block of 8 >= multiplicity"""
    lam = np.concatenate(([10, 10, 10], np.linspace(7, 0.1, 57)))
    res = largest_eigenpairs(matvec_of(np.diag(lam)), NumpyOps(), 60, 5, rng=np.random.default_rng(2))
    np.testing.assert_allclose(res.values, lam[:5], rtol=0, atol=1e-13)


def test_low_rank_terminates_by_exhaustion():
    rng = np.random.default_rng(3)
    U = np.linalg.qr(rng.standard_normal((40, 5)))[0]
    A = (U * np.array([5., 4, 3, 2, 1])) @ U.T
    mv = matvec_of(A)
    res = largest_eigenpairs(mv, NumpyOps(), 40, 5, rng=rng)
    assert res.exhausted
    assert res.matvecs == mv.count[0] <= 24
    np.testing.assert_allclose(res.values, [5, 4, 3, 2, 1], rtol=0, atol=1e-14)


def test_locked_vectors_give_the_next_ones():
    A, lam, U = spd(60, 4)
    res = largest_eigenpairs(matvec_of(A), NumpyOps(), 60, 4, rng=np.random.default_rng(5),
                             locked=np.ascontiguousarray(U[:, :3].T))
    np.testing.assert_allclose(res.values, lam[3:7], rtol=0, atol=1e-13 * lam[0])
    assert np.abs(np.asarray(res.vectors) @ U[:, :3]).max() < 1e-10


def test_forced_restart_agrees_with_uncapped():
    A, lam, _ = spd(200, 6, decay=0.97)
    free = largest_eigenpairs(matvec_of(A), NumpyOps(), 200, 6, rng=np.random.default_rng(7), max_basis=200)
    capped = largest_eigenpairs(matvec_of(A), NumpyOps(), 200, 6, rng=np.random.default_rng(7), max_basis=32)
    assert free.restarts == 0 and capped.restarts > 0
    tol = fixture_tol()
    assert np.abs(capped.values - free.values).max() <= tol * lam[0]
    assert np.abs(free.values - lam[:6]).max() <= tol * lam[0]


def test_seeded_run_reproduces():
    import nifty_amd as ift
    A, _, _ = spd(50, 8)
    out = []
    for _ in range(2):
        with ift.random.Context(11):
            out.append(largest_eigenpairs(matvec_of(A), NumpyOps(), 50, 3))
    assert np.array_equal(out[0].values, out[1].values)
    assert np.array_equal(np.asarray(out[0].vectors), np.asarray(out[1].vectors))


def test_no_convergence_raises_with_count():
    """the budget is 10 n matvecs; shrunk here through the solver's dimension
    count so that a slowly converging spectrum runs into it"""
    import nifty_amd.minimization.block_lanczos as bl
    A, _, _ = spd(120, 9, decay=0.999)
    s = bl._Solver(matvec_of(A), NumpyOps(), 120, 8, 0., None, np.random.default_rng(1), 1, 20, None)
    s.n_eff = 3          # a budget of 30 matvecs
    with pytest.raises(RuntimeError, match=r"no convergence within 30 matvecs \(\d+ of 8 eigenpairs converged\)"):
        s.run()


def test_bad_requests():
    A, _, _ = spd(10, 10)
    with pytest.raises(ValueError):
        largest_eigenpairs(matvec_of(A), NumpyOps(), 10, 11, rng=np.random.default_rng(0))
    with pytest.raises(ValueError):
        largest_eigenpairs(matvec_of(A), NumpyOps(), 10, 0, rng=np.random.default_rng(0))


# ------------------------------------------------- batching and statistics
class _Dense:
    """what metric_spectrum needs of a matvec, for a host matrix L"""

    def __init__(self, L):
        self.L, self.n, self.support = L, L.shape[0], None
        self.asked = []

    def explicit(self):
        return self.L

    def solver(self, nev, nlocked):
        self.asked.append((nev, nlocked))
        if not hasattr(self, "store"):
            self.store = np.zeros((self.n, self.n))
        res = largest_eigenpairs(matvec_of(self.L), NumpyOps(), self.n, nev, rng=np.random.default_rng(nlocked),
                                 locked=self.store[:nlocked] if nlocked else None)
        self.store[nlocked:nlocked + nev] = res.vectors
        return res


def dense12():
    rng = np.random.default_rng(12)
    U = np.linalg.qr(rng.standard_normal((12, 12)))[0]
    lam = np.array([900., 400, 150, 60, 20, 6, 1.5, 0.3, 0.05, 0., 0., 0.])
    return (U * lam) @ U.T


def test_batch_sizes_are_the_references():
    assert batch_sizes(16, 4) == [4, 4, 4, 4]
    assert batch_sizes(12, 5) == [2, 2, 2, 2, 4]
    assert batch_sizes(7, 2) == [3, 4]
    assert batch_sizes(20, 10) == [2] * 10


def test_batches_early_stop_and_statistics_12x12():
    L = dense12()
    want = 1.0 + np.linalg.eigvalsh(L)[::-1]
    # 7 of 9 relevant eigenvalues in batches of 2, 2, 3
    M = _Dense(L)
    ev = metric_spectrum(M, 1.0, 7, 9, min_lh_eval=1e-3, batch_number=3, verbose=False, solver=M.solver)
    assert M.asked == [(2, 0), (2, 2), (3, 4)]
    np.testing.assert_allclose(ev, want[:7], rtol=0, atol=1e-12 * want[0])
    # the early stop: |1 - min| < min_lh_eval is first true after the second batch
    M = _Dense(L)
    ev = metric_spectrum(M, 1.0, 7, 9, min_lh_eval=want[3] - 1.0 + 1e-6, batch_number=3, verbose=False,
                         solver=M.solver)
    assert M.asked == [(2, 0), (2, 2)] and ev.size == 4
    # the exact branch: all 9 relevant ones from the explicit matrix
    ev9 = metric_spectrum(_Dense(L), 1.0, 9, 9, verbose=False)
    np.testing.assert_allclose(ev9, want[:9], rtol=0, atol=1e-12 * want[0])
    with pytest.raises(ValueError, match="exceeds the number of relevant degrees of freedom"):
        metric_spectrum(_Dense(L), 1.0, 10, 9, verbose=False)
    # the statistics arithmetic (evidence_lower_bound.py:236-240) by hand
    post, lower = elbo_statistics(want[:7], 9, 12)
    assert post == pytest.approx(-0.5 * np.log(want[:7]).sum() + 6.0, rel=1e-15)
    assert lower == pytest.approx(0.5 * 2 * np.log(want[6]), rel=1e-15)


def test_distributed_ranks_share_rank_zeros_spectrum():
    """each rank solves from its own start vectors; the statistics need one
    posterior contribution, so rank 0's eigenvalues are broadcast"""
    class Comm:
        def __init__(self, size):
            self.size, self.sent = size, []

        def Get_size(self):
            return self.size

        def bcast(self, obj, root=0):
            self.sent.append((np.array(obj), root))
            return np.array([3.0, 2.0])          # what rank 0 holds

    mine = np.array([3.0 + 4e-16, 2.0])
    assert shared_spectrum(mine, None) is mine
    one = Comm(1)
    assert shared_spectrum(mine, one) is mine and not one.sent
    two = Comm(2)
    got = shared_spectrum(mine, two)
    assert np.array_equal(got, [3.0, 2.0]) and len(two.sent) == 1 and two.sent[0][1] == 0
