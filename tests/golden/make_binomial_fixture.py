"""
Generates tests/golden/reference_vectors_binomial.npz by IMPORTING THE REFERENCE (/root/reference, read-only) in this container.

Run here only (the reference never travels to the GPU box):   python tests/golden/make_binomial_fixture.py

The reference names a binomial model in the docstring of _SparsePGRegressionBase (regression.py:463-466) and defines every count
model by the three hooks a_func / b_func / c_func (:479-489); it does not ship the class.  This script defines it the way the
reference's own subclasses are written -- the hooks and `mean` on top of the reference's base class -- and records what the
reference's code does with it.  The import shims and the tape of random inputs are make_fixtures.py's (imported, not copied):
  * pypolyagamma.pgdrawvpar -> fills omega from an array this script chose, and records the b vector it was handed
  * sample_discrete_from_log / sample_gaussian / npr.permutation -> inputs taken from recorded lists
Every array saved is an INPUT or an OUTPUT of a reference function; no reference source text is stored.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_fixtures as mf           # noqa: E402  (shims, tape, omega stand-in)

OUT = mf.OUT


def main():
    mf._install_shims()
    import numpy.random as npr
    from scipy.special import gammaln
    import pypolyagamma as ppg
    import pyglm.regression as refreg
    from pyglm.regression import _SparsePGRegressionBase
    from pyglm.models import NonlinearAutoregressiveModel
    from pyglm.utils.basis import cosine_basis
    from pyglm.utils.utils import logistic

    class Binomial(_SparsePGRegressionBase):
        def __init__(self, N, B, n=1, **kwargs):
            self.n = n
            super(Binomial, self).__init__(N, B, **kwargs)

        def a_func(self, y):
            return y

        def b_func(self, y):
            return self.n * np.ones_like(y, dtype=float)

        def c_func(self, y):
            return np.exp(gammaln(self.n + 1) - gammaln(y + 1) - gammaln(self.n - y + 1))

        def mean(self, X):
            return self.n * logistic(self.activation(X))

    handed_b = []
    shim_draw = ppg.pgdrawvpar

    def recording_draw(ppgs, b, z, out):
        handed_b.append(np.array(b, dtype=float))
        shim_draw(ppgs, b, z, out)
    ppg.pgdrawvpar = recording_draw

    rng = np.random.default_rng(20261016)
    out = {}
    TAPE = mf.TAPE
    # ---- one regression: two shapes, sparse and dense
    for tag, (N, B, T, n, rho) in {"b0": (5, 2, 400, 3, 0.5), "b1": (5, 2, 400, 12, 1.0)}.items():
        np.random.seed(17)
        reg = Binomial(N, B, n=n, rho=rho, S_w=2.0, mu_w=0.0, mu_b=-0.5, S_b=1.0)
        X = np.abs(rng.standard_normal((T, N, B))) * 0.3
        y = rng.binomial(n, 0.35, size=T).astype(float)
        out[tag + "_n"] = np.array(n)
        out[tag + "_rho"], out[tag + "_mu_w"], out[tag + "_S_w"] = reg.rho.copy(), reg.mu_w.copy(), reg.S_w.copy()
        out[tag + "_mu_b"], out[tag + "_S_b"] = reg.mu_b.copy(), reg.S_b.copy()
        out[tag + "_X"], out[tag + "_y"] = X, y
        out[tag + "_a0"], out[tag + "_W0"], out[tag + "_b0"] = reg.a.copy(), reg.W.copy(), reg.b.copy()
        psi = reg.activation(X)
        out[tag + "_psi"], out[tag + "_kappa"], out[tag + "_mean"] = psi, reg.kappa(X, y), reg.mean(X)
        out[tag + "_ll"] = reg.log_likelihood((X, y))
        om = mf.pg_moment_matched(psi, rng) * n
        perm = rng.permutation(N)
        u = rng.random(N)
        z = rng.standard_normal(N * B + 1)
        orig_perm = npr.permutation
        refreg.npr.permutation = lambda k: perm.copy()
        TAPE.omega = [om.copy()]
        TAPE.uniforms = list(u)
        TAPE.used_u, TAPE.used_z = [], []

        class LazyNormals(object):
            def pop(self, i=0):
                return z[:int(reg.a.sum()) * B + 1].copy()
        TAPE.normals = LazyNormals()
        del handed_b[:]
        reg.resample([(X, y)])
        refreg.npr.permutation = orig_perm
        assert len(handed_b) == 1
        out[tag + "_pg_b"], out[tag + "_om"] = handed_b[0], om
        out[tag + "_perm"], out[tag + "_u"], out[tag + "_z"] = perm, u, z
        out[tag + "_a1"], out[tag + "_W1"], out[tag + "_b1"] = reg.a.copy(), reg.W.copy(), reg.b.copy()
        out[tag + "_ll1"] = reg.log_likelihood((X, y)).sum()

    # ---- model level: the reference's loop (models.py:169-171) over four binomial regressions, n = 4, randomness injected
    np.random.seed(5)
    N, B, L, T, n = 4, 2, 20, 600, 4
    basis = cosine_basis(B, L=L) / L
    regs = [Binomial(N, B, n=n, S_w=4.0, mu_b=-1.0) for _ in range(N)]
    glm = NonlinearAutoregressiveModel(N, regs, basis=basis)
    Y = rng.binomial(n, 0.2, size=(T, N)).astype(float)
    glm.add_data(Y)
    Xm = glm.data_list[0][0]
    out["M_n"], out["M_basis"], out["M_Y"], out["M_X"] = np.array(n), basis, Y, Xm
    out["M_A0"], out["M_W0"], out["M_b0"] = glm.adjacency.copy(), glm.weights.copy(), glm.biases.copy()
    out["M_ll0"] = np.array(glm.log_likelihood())
    perms = np.array([rng.permutation(N) for _ in range(N)])
    us = rng.random((N, N))
    zs = rng.standard_normal((N, N * B + 1))
    oms = np.array([mf.pg_moment_matched(glm.regressions[k].activation(Xm), rng) * n for k in range(N)])
    out["M_perms"], out["M_us"], out["M_zs"], out["M_omegas"] = perms, us, zs, oms
    state = dict(n=0)
    orig_perm = npr.permutation
    refreg.npr.permutation = lambda k: perms[state["n"]].copy()

    class ModelNormals(object):
        def pop(self, i=0):
            r = glm.regressions[state["n"]]
            return zs[state["n"], :int(r.a.sum()) * B + 1].copy()
    TAPE.normals = ModelNormals()
    for k, reg in enumerate(glm.regressions):
        state["n"] = k
        TAPE.omega = [oms[k].copy()]
        TAPE.uniforms = list(us[k])
        reg.resample([(X_, Y_[:, k]) for (X_, Y_) in glm.data_list])
    refreg.npr.permutation = orig_perm
    out["M_A1"], out["M_W1"], out["M_b1"] = glm.adjacency.copy(), glm.weights.copy(), glm.biases.copy()
    out["M_ll1"] = np.array(glm.log_likelihood())

    path = os.path.join(OUT, "reference_vectors_binomial.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, "%d arrays, %.1f KB" % (len(out), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
