"""Plain NumPy references, in np.longdouble, of the pieces of dense linear algebra behind a sweep: the weight draw (an upper Cholesky and
two triangular solves, pyglm/regression.py:323-340), the sweep tableau of the collapsed flips (pgl_flips.hip, header) and the serial loop of
proposals on it (pyglm/regression.py:282-320).  No GPU, no library call: tests/test_dense_ref_host.py checks these functions against their own
defining identities, tests/test_gpu_chol.py, tests/test_gpu_tableau.py and tests/test_gpu_flip_windows.py hold the kernels to them.

Every bound the GPU tests use is the forward-error bound of the operation, computed from the reference's own matrix:
    8 * n * 2^-53 * kappa_2(pivot / active block),     kappa_2 from np.linalg.cond of the fp64 copy
-- 8 is the one free constant (blocked summation order against the bound's leading term)."""
import numpy as np

LD = np.longdouble
U53 = 2.0 ** -53


def ld(x):
    return np.asarray(x, dtype=LD)


# ------------------------------------------------------------------------------------------------------------ Cholesky and the draw
def chol_upper(J, block=48):
    """U upper triangular with U'U = J (J symmetric positive definite; only its upper triangle is read), in longdouble.  Right-looking on
    `block`-wide panels so that the n^3 / 3 multiply-adds run inside NumPy's matmul instead of a Python loop per column."""
    A = np.triu(ld(J)).copy()
    n = A.shape[0]
    for q in range(0, n, block):
        e = min(q + block, n)
        for j in range(q, e):                           # the diagonal block and its row panel, row by row
            d = A[j, j]
            if not d > 0:
                raise np.linalg.LinAlgError("not positive definite at row %d" % j)
            A[j, j:] /= np.sqrt(d)
            if j + 1 < e:
                A[j + 1:e, j + 1:] -= np.outer(A[j, j + 1:e], A[j, j + 1:])
        if e < n:
            P = A[q:e, e:]
            A[e:, e:] -= np.triu(P.T @ P)
    return np.triu(A)


def solve_upper(U, r):
    """v with U v = r (back substitution); r a vector or a matrix of right-hand sides"""
    U, v = ld(U), ld(r).copy()
    for i in range(U.shape[0] - 1, -1, -1):
        v[i] /= U[i, i]
        v[:i] -= np.multiply.outer(U[:i, i], v[i])
    return v


def solve_upper_t(U, r):
    """w with U' w = r (forward substitution); r a vector or a matrix of right-hand sides"""
    U, w = ld(U), ld(r).copy()
    n = U.shape[0]
    for i in range(n):
        w[i] /= U[i, i]
        w[i + 1:] -= np.multiply.outer(U[i, i + 1:], w[i])
    return w


def inv_spd(J):
    """J^-1 = U^-1 U^-T of a symmetric positive definite J through its longdouble factor"""
    U = chol_upper(J)
    P = solve_upper(U, solve_upper_t(U, np.eye(U.shape[0], dtype=LD)))
    return (P + P.T) / 2


def draw_from_factor(U, h, z):
    """(mu, x - mu) = (J^-1 h, U^-1 z) for J = U'U"""
    return solve_upper(U, solve_upper_t(U, h)), solve_upper(U, z)


def draw(J_aa, h_a, z):
    """mu = J_aa^-1 h_a and x = mu + U^-1 z with U'U = J_aa: the law of sample_gaussian(J=, h=) at pyglm/regression.py:323-340"""
    mu, dx = draw_from_factor(chol_upper(J_aa), h_a, z)
    return mu, mu + dx


def bordered_prefix_factor(U_full, w_full, d, k):
    """Factor of [[J_kk, j], [j', d]] from U_full'U_full = J (any leading block of it) and w_full = U_full^-T j_full: the factor of a leading
    block is the leading block of the factor, and forward substitution is prefix-consistent, so one factorisation serves every nested
    prefix.  Returns the (k + 1)-square upper factor."""
    U = np.zeros((k + 1, k + 1), dtype=LD)
    U[:k, :k] = U_full[:k, :k]
    U[:k, k] = w_full[:k]
    s = ld(d) - w_full[:k] @ w_full[:k]
    if not s > 0:
        raise np.linalg.LinAlgError("bordered block not positive definite")
    U[k, k] = np.sqrt(s)
    return U


# ------------------------------------------------------------------------------------------------------------ the sweep tableau
def sweep(M, idx, sign):
    """Sequential single-pivot symmetric sweeps of the full symmetric matrix M on the rows idx[q] (sign[q] = +1 forward, -1 reverse):
        d = M_pp;   M_ij -= M_ip M_pj / d (i, j != p);   M_ip = M_pi = sign M_ip / d;   M_pp = -1 / d."""
    return sweep_prefixes(M, idx, sign, [len(idx)])[len(idx)]


def sweep_prefixes(M, idx, sign, counts):
    """{k: the tableau after the first k pivots of the list} for k in counts -- the sweeps are sequential, so one pass over the longest list
    gives the reference of every list that is a prefix of it"""
    M = ld(M).copy()
    buf = np.empty_like(M)
    want, out = set(int(k) for k in counts), {}
    if 0 in want:
        out[0] = M.copy()
    for q, (p, s) in enumerate(zip(np.asarray(idx, dtype=int), np.asarray(sign, dtype=float))):
        d = M[p, p]
        col = M[:, p].copy()
        np.multiply(col[:, None], (col / d)[None, :], out=buf)   # (two passes over M per pivot: longdouble arithmetic is the cost here)
        M -= buf
        M[p, :] = M[:, p] = LD(s) * col / d
        M[p, p] = -1 / d
        if q + 1 in want:
            out[q + 1] = M.copy()
    return out


def sweep_block(M, idx, sign):
    """The block formula of pgl_flips.hip's header on the pivot set D = idx, R = the rest:
        G = M_DD^-1;   M_RR -= M_RD G M_DR;   M_RD = M_RD G Sg;   M_DD = -Sg G Sg      (Sg = diag(sign))"""
    M = ld(M).copy()
    idx = np.asarray(idx, dtype=int)
    sg = ld(sign)
    rest = np.setdiff1d(np.arange(M.shape[0]), idx)
    G = inv_sym(M[np.ix_(idx, idx)])
    RD = M[np.ix_(rest, idx)]
    M[np.ix_(rest, rest)] -= RD @ G @ RD.T
    M[np.ix_(rest, idx)] = (RD @ G) * sg[None, :]
    M[np.ix_(idx, rest)] = M[np.ix_(rest, idx)].T
    M[np.ix_(idx, idx)] = -(sg[:, None] * G * sg[None, :])
    return M


def inv_sym(A):
    """inverse of a symmetric matrix with non-zero leading pivots (definite or a swept, quasi-definite block) by Gauss-Jordan in longdouble"""
    A = ld(A).copy()
    n = A.shape[0]
    X = np.eye(n, dtype=LD)
    for p in range(n):
        d = A[p, p]
        A[p] /= d
        X[p] /= d
        f = A[:, p].copy()
        f[p] = 0
        A -= np.outer(f, A[p])
        X -= np.outer(f, X[p])
    return (X + X.T) / 2


def scale_swept(M, piv, c):
    """the tableau of c A swept on the rows piv, from M = A swept on the same rows: G = (c A_DD)^-1 = G / c, so the non-pivot square scales by
    c, the pivot rows and columns outside the pivot block not at all, the pivot block by 1 / c.  For c a power of two the scaled sweep is the
    same arithmetic with shifted exponents: the result is exact, and one reference sweep serves neurons whose tableaux differ by such a c."""
    piv = np.asarray(piv, dtype=int)
    out = ld(M) * LD(c)
    out[:, piv] = M[:, piv]
    out[piv, :] = M[piv, :]
    out[np.ix_(piv, piv)] = M[np.ix_(piv, piv)] / LD(c)
    return out


def tableau(J, h):
    """A = [[J, h], [h', 0]]"""
    n = J.shape[0]
    A = np.zeros((n + 1, n + 1), dtype=LD)
    A[:n, :n] = ld(J)
    A[:n, n] = A[n, :n] = ld(h)
    return A


# ------------------------------------------------------------------------------------------------------------ the collapsed proposals
def block_dml(M, blk, on):
    """change in log marginal likelihood for switching the block with rows blk ON, read off the tableau M, without the prior term c0
    (pgl_flips.hip, header): Q = M[blk, blk] (minus it when the block is on), v = M[blk, D + 1];  (on ? +1/2 : -1/2) log|Q| + 1/2 v'Q^-1 v"""
    Q = M[np.ix_(blk, blk)]
    U = chol_upper(-Q if on else Q)
    logdet = 2 * np.sum(np.log(np.diag(U)))
    w = solve_upper_t(U, M[blk, M.shape[0] - 1])
    return (logdet if on else -logdet) / 2 + (w @ w) / 2


def flip_proposals(M, a, perm, u, rho, c0, B, R=None):
    """The collapsed proposals of pyglm/regression.py:282-320 run serially on the full tableau M (symmetric, (N B + 2)-square, rows in J's
    order, swept on {bias} U {blocks with a on}): step k proposes block m = perm[k] with the uniform u[k];
        d = block_dml + c0[m] + log rho[m] - log(1 - rho[m]);   v = [u[k] (e0 + e1) > e0],  e0 = exp(-max(d, 0)),  e1 = exp(d - max(d, 0))
    -- for rho exactly 0 or 1 the log-odds are NaN and v = 0 (the reference's 0 log 0 reaching sample_discrete_from_log) -- and a decision
    that differs from a[m] sweeps the block's rows (forward when switched on).  u, rho, c0 are read as they are given (fp64 values).
    Returns a dict: logodds, decision, threshold = 1 / (1 + exp(d)) per step (the decision is u > threshold), flips = [(k, m, +1 | -1)],
    M and a at the end, and snaps = [(M, a) after every R steps and after the last] when R is given."""
    M, a = ld(M).copy(), np.asarray(a).astype(bool).copy()
    N = len(perm)
    lo, thr, dec, flips, snaps = np.full(N, np.nan, dtype=LD), np.full(N, np.nan, dtype=LD), np.zeros(N, dtype=int), [], []
    for k in range(N):
        m = int(perm[k])
        blk = np.arange(m * B, (m + 1) * B)
        if 0 < rho[m] < 1:
            d = block_dml(M, blk, a[m]) + LD(c0[m]) + np.log(LD(rho[m])) - np.log(1 - LD(rho[m]))
            mx = max(d, LD(0))
            e0, e1 = np.exp(-mx), np.exp(d - mx)
            lo[k], thr[k], dec[k] = d, 1 / (1 + np.exp(d)), int(LD(u[k]) * (e0 + e1) > e0)
        if dec[k] != int(a[m]):
            s = 1 if dec[k] else -1
            M = sweep(M, blk, s * np.ones(B))
            a[m] = bool(dec[k])
            flips.append((k, m, s))
        if R and ((k + 1) % R == 0 or k == N - 1):
            snaps.append((M.copy(), a.copy()))
    return dict(logodds=lo, decision=dec, threshold=thr, flips=flips, M=M, a=a, snaps=snaps)


def position_order(M, perm, B):
    """the tableau in visit order: block perm[k] at position k, the bias and potential rows last (what pgl_flip_visit_order builds)"""
    perm = np.asarray(perm, dtype=int)
    D = len(perm) * B
    rows = np.concatenate([(perm[:, None] * B + np.arange(B)[None, :]).ravel(), [D, D + 1]])
    return M[np.ix_(rows, rows)]


# ------------------------------------------------------------------------------------------------------------ test matrices
def wellcond_system(n, rng):
    """J = X'X / T + I with X (2n x n) standard normal (kappa_2 about 3.6 at n = 400 and 800) and a random h; fp64"""
    X = rng.standard_normal((2 * n, n))
    J = X.T @ X / (2 * n) + np.eye(n)
    return (J + J.T) / 2, rng.standard_normal(n)


def spectrum_system(n, kappa, rng):
    """J = Q diag(lam) Q' with lam log-spaced from 1 / kappa to 1 (kappa_2 = kappa by construction) and a random h; fp64"""
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = np.logspace(-np.log10(kappa), 0.0, n) if n > 1 else np.ones(1)
    J = (Q * lam[None, :]) @ Q.T
    return (J + J.T) / 2, rng.standard_normal(n)


def bound(n, block64):
    """8 n 2^-53 kappa_2(block), kappa_2 by np.linalg.cond of the fp64 copy"""
    return 8.0 * n * U53 * float(np.linalg.cond(np.asarray(block64, dtype=np.float64)))


def relerr(dev, ref):
    """max |dev - ref| / max |ref| (dev fp64, ref longdouble); NaN in dev gives inf"""
    ref = ld(ref)
    d = np.abs(ld(dev) - ref)
    if not np.all(np.isfinite(np.asarray(dev, dtype=np.float64))):
        return np.inf
    m = np.max(np.abs(ref)) if ref.size else LD(0)
    return float(np.max(d) / m) if ref.size and m > 0 else float(np.max(d)) if ref.size else 0.0
