"""Block Lanczos for the largest eigenpairs of a symmetric positive
semi-definite operator held on the device.

What the reference gets from ARPACK on the host, one matvec at a time
(src/evidence_lower_bound.py:93, scipy.sparse.linalg.eigsh), here runs on
blocks of up to 8 vectors: the matvec is the batched fused metric, and the
orthogonalisation against the growing basis -- the part that streams m * n
doubles -- is two native kernels (csrc/nft_eig.hip):

  dots(V, W)            C = V W^T                      nft_gram_dots
  axpy(V, T, W, beta)   W = beta W + T^T V             nft_gram_axpy

Algorithm
---------
Q holds an orthonormal basis, row-wise.  One step takes the newest block Q_j
(kb <= `block` rows), forms W = A Q_j and removes, by two passes of classical
Gram-Schmidt, its components along the locked vectors and along every basis
row.  The summed coefficients of the two passes against the basis are column
block j of the projected matrix T = Q A Q^T, which is therefore a plain
symmetric matrix assembled from measured inner products: no three-term
recurrence is assumed, so T stays valid after a restart and with refilled
columns.  What is left of W is orthonormalised through its kb x kb Gram matrix
(host eigh, the same two kernels) and becomes block j + 1; its coefficients
`Cn` (next block against A Q) give the residual estimate ||Cn y|| of a Ritz
pair (theta, y) of T.

Convergence is ARPACK's criterion for symmetric problems: ||Cn y|| <= tol *
max(eps^(2/3), |theta|), tol = 0 meaning eps.

Breakdown: a block loses rank when the Krylov space is exhausted (J^T W J has
rank <= ndata; degenerate spectra).  Rows of W below `100 eps ||A||` are
dropped (their coupling is exactly zero) and the block is refilled with fresh
random vectors orthogonalised against everything held.  Once that has happened
the wanted pairs alone no longer certify the result -- a copy of a degenerate
eigenvalue beyond the block size lives outside the exhausted space -- so the
solver then also requires (a) every unconverged Ritz pair to lie below the
wanted ones by more than its residual and (b) after a total breakdown, that
the block just multiplied held a fresh vector: a random vector of the
complement that A maps into the held space shows, with probability one, that
A is a multiple of the identity on that complement.

Thick restart: when the next block would not fit into the basis buffer, the
wanted Ritz vectors plus a few are formed (axpy with beta = 0), T becomes
their diagonal, and the next block is kept; its column of T is measured like
any other when it is multiplied.  Forming Ritz vectors adds round-off to the
basis' orthonormality at every restart, so the kept vectors are put right
through their Gram matrix (G^-1/2, the same two kernels), and a run that
restarted measures the returned values afresh: one more Rayleigh-Ritz on the
nev returned vectors (nev matvecs), whose round-off is that of one measurement
instead of growing with the number of restarts.

The `ops` argument carries the array primitives.  The package supplies
NativeOps only (device tensors, the HIP kernels); the CPU tests pass a numpy
double in, which exercises this control logic without a GPU.  There is no
CPU fallback inside the package.
"""
import numpy as np

EPS = float(np.finfo(np.float64).eps)


class NativeOps:
    """(rows, n) fp64 device buffers and the two Gram kernels."""
    from .._native import GRAM_KMAX as kmax

    def __init__(self, device=None):
        import torch
        from .. import _native, config
        self._torch, self._native = torch, _native
        self.device = config.device() if device is None else device
        _native.load()

    def zeros(self, rows, n):
        return self._torch.zeros((rows, n), dtype=self._torch.float64, device=self.device)

    def set(self, rows, host):
        rows.copy_(self._torch.from_numpy(np.ascontiguousarray(host, dtype=np.float64)))

    def dots(self, V, W):
        """V W^T as a host (m, k) array"""
        return self._native.gram_dots(V, W).cpu().numpy()

    def axpy(self, V, T, W, beta):
        """W = beta W + T^T V in place; T a host (m, k) array"""
        Td = self._torch.from_numpy(np.ascontiguousarray(T, dtype=np.float64)).to(self.device)
        self._native.gram_axpy(V, Td, W, beta)

    def free_rows(self, n):
        """rows of n doubles in half the free device memory (the CG ring's rule)"""
        return int(self._torch.cuda.mem_get_info(self.device)[0] // 2 // (8 * n))


class EigResult:
    """values (descending), vectors ((len(values), n) rows in the ops' array
    type) and the solver's counters: matvecs, steps, refills (columns replaced
    by fresh random vectors after a loss of rank), restarts, exhausted (True
    if the run ended because the held space was invariant)."""

    def __init__(self, values, vectors, **counters):
        self.values, self.vectors = values, vectors
        self.__dict__.update(counters)


def _chunks(k, kmax):
    return [(i, min(i + kmax, k)) for i in range(0, k, kmax)]


class _Solver:
    def __init__(self, matvec, ops, n, nev, tol, locked, rng, block, max_basis, support):
        self.matvec, self.ops, self.n, self.nev = matvec, ops, int(n), int(nev)
        self.tol = EPS if tol == 0 else float(tol)
        self.locked = locked if locked is not None and len(locked) else None
        self.nlock = 0 if self.locked is None else len(self.locked)
        self.rng = rng
        self.support = None if support is None else np.asarray(support, dtype=np.float64)
        self.n_eff = self.n if support is None else int(np.count_nonzero(support))
        self.room = self.n_eff - self.nlock          # dimension of the space searched
        if self.nev < 1 or self.nev > self.room:
            raise ValueError(f"nev = {nev} eigenpairs asked of a space of dimension {self.room}")
        kmax = getattr(ops, "kmax", 8)
        self.block = max(1, min(int(block), kmax, self.room))
        want = max(3 * self.nev, self.nev + 8 * self.block)
        cap = min(want, self.room)
        if max_basis is not None:
            cap = min(int(max_basis), self.room)
        elif hasattr(ops, "free_rows"):
            # basis + restart scratch + two work blocks inside the memory cap
            cap = min(cap, (ops.free_rows(self.n) - 2 * self.block) // 2)
        self.keep_extra = max(self.block, min(self.nev // 2, 16))
        need = min(self.room, self.nev + self.keep_extra + 2 * self.block)
        if cap < need:
            raise ValueError(f"a basis of {cap} vectors cannot hold {self.nev} wanted pairs and two blocks of "
                             f"{self.block} ({need} needed)")
        self.cap = cap
        self.Q = ops.zeros(cap, self.n)
        self.W = ops.zeros(self.block, self.n)
        self.S = ops.zeros(self.block, self.n)
        self.Z = None
        self.T = np.zeros((cap, cap))
        self.anorm = 0.0
        self.matvecs = self.steps = self.refills = self.restarts = 0
        self.broken = False

    # ------------------------------------------------------------ pieces
    def _project(self, X, mheld, passes):
        """X -= (locked, Q[:mheld]) components, `passes` times; returns the
        summed coefficients against Q[:mheld] ((mheld, rows) host array)"""
        ops, C = self.ops, np.zeros((mheld, len(X)))
        for _ in range(passes):
            if self.locked is not None:
                ops.axpy(self.locked, -ops.dots(self.locked, X), X, 1.0)
            if mheld:
                c = ops.dots(self.Q[:mheld], X)
                ops.axpy(self.Q[:mheld], -c, X, 1.0)
                C += c
        return C

    def _orthonormalise(self, X, mheld, floor):
        """the rows of X, already projected, orthonormalised into Q[mheld:]:
        Gram matrix -> host eigh -> directions of norm <= floor dropped -> one
        more projection -> symmetric normalisation.  Returns (r, B) with X =
        B^T Q[mheld:mheld + r] up to the dropped part."""
        ops, kb = self.ops, len(X)
        G = ops.dots(X, X)
        s, U = np.linalg.eigh(0.5 * (G + G.T))
        s, U = s[::-1], U[:, ::-1]
        r = int(np.count_nonzero(np.sqrt(np.maximum(s, 0.0)) > floor))
        r = min(r, self.cap - mheld, self.room - mheld)
        while r > 0:
            rt = np.sqrt(s[:r])
            Y = self.S[:r]
            ops.axpy(X, U[:, :r] / rt, Y, 0.0)
            self._project(Y, mheld, 1)
            G2 = ops.dots(Y, Y)
            s2, U2 = np.linalg.eigh(0.5 * (G2 + G2.T))
            if s2[0] >= 0.25:
                ops.axpy(Y, (U2 / np.sqrt(s2)) @ U2.T, self.Q[mheld:mheld + r], 0.0)
                return r, ((U2 * np.sqrt(s2)) @ U2.T) @ (rt[:, None] * U[:, :r].T)
            r -= 1      # the weakest direction was noise of the projection after all
        return 0, np.zeros((0, kb))

    def _fresh(self, mheld, count):
        """up to `count` fresh random unit vectors orthogonal to everything
        held, written to Q[mheld:]; returns how many were found"""
        count = min(count, self.cap - mheld, self.room - mheld)
        if count <= 0:
            return 0
        x = self.rng.normal(0.0, 1.0, (count, self.n))
        if self.support is not None:
            x *= self.support
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        X = self.W[:count]
        self.ops.set(X, x)
        self._project(X, mheld, 2)
        # a random unit vector keeps a fair share of its norm unless the
        # complement is (numerically) empty
        r, _ = self._orthonormalise(X, mheld, 1e-6)
        self.refills += r
        return r

    def _ritz(self, m, Cn):
        """Ritz pairs of T[:m, :m], descending, and their residual estimates"""
        th, Y = np.linalg.eigh(self.T[:m, :m])
        th, Y = th[::-1], Y[:, ::-1]
        res = np.linalg.norm(Cn @ Y, axis=0) if Cn.shape[0] else np.zeros(m)
        return th, Y, res

    def _converged(self, th, res):
        return res <= self.tol * np.maximum(EPS ** (2. / 3.), np.abs(th))

    def _vectors(self, Y, m, out):
        """out[i] = sum_j Y[j, i] Q[j]  (Ritz vectors, chunks of kmax)"""
        for a, b in _chunks(Y.shape[1], getattr(self.ops, "kmax", 8)):
            self.ops.axpy(self.Q[:m], Y[:, a:b], out[a:b], 0.0)

    def _inv_sqrt_gram(self, X):
        """G^-1/2 (symmetric) of the Gram matrix G = X X^T of nearly orthonormal rows"""
        k = len(X)
        G = np.zeros((k, k))
        for a, b in _chunks(k, getattr(self.ops, "kmax", 8)):
            G[:, a:b] = self.ops.dots(X, X[a:b])
        g, U = np.linalg.eigh(0.5 * (G + G.T))
        return (U / np.sqrt(g)) @ U.T

    def _restart(self, m, knext, th, Y):
        """keep the leading Ritz vectors and the next block (rows m:m+knext)"""
        p = min(self.nev + self.keep_extra, m)
        if self.Z is None:
            self.Z = self.ops.zeros(min(self.nev + self.keep_extra, self.cap), self.n)
        self._vectors(Y[:, :p], m, self.Z[:p])
        nxt = self.S[:knext]
        nxt[:] = self.Q[m:m + knext]
        # Z = Y^T Q inherits Q's departure from orthonormality and adds its own
        # round-off, restart after restart: put it right through Z's Gram
        # matrix, Q[:p] = G^-1/2 Z (T stays diag(theta): the change is of the order
        # of its round-off, and the returned values are measured afresh, _refresh)
        S = self._inv_sqrt_gram(self.Z[:p])
        for a, b in _chunks(p, getattr(self.ops, "kmax", 8)):
            self.ops.axpy(self.Z[:p], S[:, a:b], self.Q[a:b], 0.0)
        self.Q[p:p + knext] = nxt
        self.T[:] = 0.0
        self.T[np.arange(p), np.arange(p)] = th[:p]
        self.restarts += 1
        return p

    # -------------------------------------------------------------- run
    def _refresh(self, vec):
        """Rayleigh-Ritz on the k returned vectors themselves: H = vec A vec^T
        measured with k more matvecs.  After restarts T's kept part is the
        diagonal of earlier Ritz values, so its round-off grows with the
        number of restarts; H carries that of one measurement only."""
        ops, k = self.ops, len(vec)
        kmax = getattr(ops, "kmax", 8)
        H = np.zeros((k, k))
        for a, b in _chunks(k, kmax):
            W = self.W[:b - a]
            self.matvec(vec[a:b], W)
            self.matvecs += b - a
            H[:, a:b] = ops.dots(vec, W)
        S = self._inv_sqrt_gram(vec)
        th, Y = np.linalg.eigh(S @ (0.5 * (H + H.T)) @ S)
        th, Y = th[::-1], S @ Y[:, ::-1]
        out = ops.zeros(k, self.n)
        for a, b in _chunks(k, kmax):
            ops.axpy(vec, Y[:, a:b], out[a:b], 0.0)
        return th, out

    def _result(self, th, Y, res, m, exhausted):
        k = min(self.nev, m)
        vec = self.ops.zeros(k, self.n)
        self._vectors(Y[:, :k], m, vec)
        th = th[:k].copy()
        if self.restarts:
            th, vec = self._refresh(vec)
        return EigResult(th, vec, matvecs=self.matvecs, steps=self.steps, refills=self.refills,
                         restarts=self.restarts, exhausted=bool(exhausted), residuals=res[:k].copy())

    def run(self):
        nev, block = self.nev, self.block
        m = 0                                  # rows of Q whose column of T is measured
        kb = self._fresh(0, block)             # the block Q[m:m + kb] to multiply next
        self.refills = 0                       # the start block is no refill
        nfresh = 0                             # fresh vectors in that block
        if kb == 0:
            raise RuntimeError("block Lanczos: no start vector outside the locked space")
        limit = 10 * self.n_eff
        nconv, th, Y = 0, None, None
        while True:
            if self.matvecs + kb > limit:
                raise RuntimeError(f"block Lanczos: no convergence within {limit} matvecs "
                                   f"({nconv} of {nev} eigenpairs converged)")
            # this block and the next one must fit, else thick restart
            if m and self.cap < self.room and m + kb + block > self.cap:
                m = self._restart(m, kb, th, Y)
            X, W = self.Q[m:m + kb], self.W[:kb]
            self.matvec(X, W)
            self.matvecs += kb
            self.steps += 1
            mh = m + kb
            C = self._project(W, mh, 2)
            self.T[:mh, m:mh] = C
            self.T[m:mh, :mh] = C.T
            blk = self.T[m:mh, m:mh]
            self.T[m:mh, m:mh] = 0.5 * (blk + blk.T)
            # ||Q A Q_j|| <= ||A||: the scale below which a row of W is noise
            self.anorm = max(self.anorm, float(np.linalg.norm(C, 2)))
            r, B = self._orthonormalise(W, mh, 100.0 * EPS * self.anorm)
            Cn = np.zeros((r, mh))
            Cn[:, m:mh] = B
            had_fresh, total = nfresh > 0, r == 0
            if r < kb:
                self.broken = True
            m = mh
            th, Y, res = self._ritz(m, Cn)
            ok = self._converged(th, res)
            nconv = int(np.count_nonzero(ok[:nev]))
            if m >= self.room:
                return self._result(th, Y, res, m, True)      # the whole space is held: T is exact
            done = m >= nev and nconv == nev
            if done and self.broken:
                un = ~ok
                done = not np.any(th[un] + res[un] > th[nev - 1]) and (had_fresh or not total)
            if done:
                return self._result(th, Y, res, m, total)
            nfresh = self._fresh(m + r, block - r) if (self.broken and r < block) else 0
            kb = r + nfresh
            if kb == 0:
                # nothing new can be found: the held space is all that can be reached
                return self._result(th, Y, res, m, True)


def largest_eigenpairs(matvec, ops, n, nev, tol=0., locked=None, rng=None, block=8, max_basis=None, support=None):
    """The `nev` largest eigenpairs of the symmetric positive semi-definite
    operator A restricted to the complement of `locked`.

    matvec(X, Y): Y[b] = A X[b] for the rows of X ((kb, n), kb <= block <= 8)
    into the rows of Y, both in the ops' array type.
    ops: zeros / set / dots / axpy and kmax (NativeOps on the device).
    locked: (l, n) orthonormal rows to stay orthogonal to, or None.
    rng: numpy Generator of the start and refill vectors (default: the
    package's current generator, so a seeded run reproduces).
    max_basis: cap of the basis in vectors (default: max(3 nev, nev + 8 block),
    within half the free device memory); reaching it triggers a thick restart.
    support: host 0/1 mask of the n elements that are degrees of freedom
    (packed layouts carry zero padding), or None for all.
    Returns an EigResult."""
    if rng is None:
        from .. import random
        rng = random.current_rng()
    return _Solver(matvec, ops, n, nev, tol, locked, rng, block, max_basis, support).run()
