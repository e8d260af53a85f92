// Stand-alone check of the host-side argument logic of pgl_simulate_offset, pgl_simulate_offset_build and pgl_latent_prior_paths under the
// host sanitizers: every refused argument set must return PGL_ERR_ARG with a message and touch nothing, whatever pointers it was given.  No
// GPU is needed: a refused call returns before the first HIP call.  The two translation units that hold the three entries are compiled
// with the sanitizers into the program itself (its definitions take precedence); the rest of the library (pgl_set_error, pgl_last_error, the
// device queries) comes from the built libpyglm_hip.so.  Build and run from the repository root, after the library:
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer -I include \
//         tools/check_simulate_offset_args.cpp pyglm_amd/csrc/pgl_generate.hip pyglm_amd/csrc/pgl_simulate_offset.hip \
//         -fsanitize=address,undefined -L pyglm_amd/lib -lpyglm_hip -Wl,-rpath,$PWD/pyglm_amd/lib -o tools/bin/check_simulate_offset_args
//   tools/bin/check_simulate_offset_args
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pyglm_hip.h"
#include "pyglm_hip_simulate_offset.h"

static int failures = 0;

static void refused(const char* what, int rc) {
    const char* msg = pgl_last_error();
    const bool ok = rc == 1 && msg && std::strstr(msg, "argument check failed");
    std::printf("%-58s rc=%d %s\n", what, rc, ok ? "refused" : "NOT REFUSED");
    if (!ok) ++failures;
}

int main() {
    // host memory stands in for device memory: a refused call must not read or write any of it (exact sizes: the sanitizer sees an overrun)
    const int N = 4, B = 1, L = 3, R = 2, Tc = 5, Q = 2, K_obs = 1;
    std::vector<double> Wm(N * N * B), bias(N), basis(L * B), par(N), ring(R * L * N), Y(R * Tc * N), sum(R * N), sumsq(R * N), Off(R * Tc * N);
    std::vector<int> kind(N), status(4);
    std::vector<char> work(pgl_simulate_work_bytes(N, B, R));
    auto sim = [&](const double* off, long ldo_t, long ldo_r, int n = N, int tc = Tc, long ldr = (long)Tc * N, long t0 = 0) {
        return pgl_simulate_offset(Wm.data(), bias.data(), basis.data(), n, B, L, kind.data(), par.data(), R, 0, 1ULL, ring.data(), Y.data(), ldr,
                                   sum.data(), sumsq.data(), t0, tc, work.data(), status.data(), off, ldo_t, ldo_r, nullptr);
    };
    refused("simulate_offset: ldo_t < N", sim(Off.data(), N - 1, (long)Tc * N));
    refused("simulate_offset: 0 < ldo_r < (Tc - 1) ldo_t + N", sim(Off.data(), N, (long)Tc * N - 1));
    refused("simulate_offset: ldo_r < 0", sim(Off.data(), N, -1));
    refused("simulate_offset: N = 0", sim(Off.data(), N, 0, 0));
    refused("simulate_offset: Tc = 0", sim(Off.data(), N, 0, N, 0));
    refused("simulate_offset: ldr < Tc N", sim(Off.data(), N, 0, N, Tc, (long)Tc * N - 1));
    refused("simulate_offset: t0 + Tc beyond 2^31", sim(Off.data(), N, 0, N, Tc, (long)Tc * N, (1L << 31) - 3));
    refused("simulate_offset: Off = NULL, Tc = 0 (pgl_simulate's checks)", sim(nullptr, 0, 0, N, 0));

    std::vector<double> S(Tc * K_obs), X(R * Tc * Q), Beta((K_obs + Q) * N);
    auto build = [&](const double* s, long lds, const double* x, long ldx_r, const double* beta, long ldn, double* off, long ldo_t, long ldo_r, int tc,
                     int n, int k_obs, int q, int r) {
        return pgl_simulate_offset_build(s, lds, x, ldx_r, beta, ldn, off, ldo_t, ldo_r, tc, n, k_obs, q, r, nullptr);
    };
    const long ldx = (long)Tc * Q, ldo = (long)Tc * N;
    refused("offset_build: Q > PGL_SIM_LATENT_MAX", build(S.data(), K_obs, X.data(), ldx, Beta.data(), N, Off.data(), N, ldo, Tc, N, K_obs, 9, R));
    refused("offset_build: K_obs + Q = 0", build(S.data(), K_obs, X.data(), ldx, Beta.data(), N, Off.data(), N, ldo, Tc, N, 0, 0, 1));
    refused("offset_build: K_obs + Q > 32", build(S.data(), 31, X.data(), ldx, Beta.data(), N, Off.data(), N, ldo, Tc, N, 31, Q, R));
    refused("offset_build: K_obs < 0", build(S.data(), K_obs, X.data(), ldx, Beta.data(), N, Off.data(), N, ldo, Tc, N, -1, Q, R));
    refused("offset_build: lds < K_obs", build(S.data(), 0, X.data(), ldx, Beta.data(), N, Off.data(), N, ldo, Tc, N, K_obs, Q, R));
    refused("offset_build: S = NULL with K_obs > 0", build(nullptr, K_obs, X.data(), ldx, Beta.data(), N, Off.data(), N, ldo, Tc, N, K_obs, Q, R));
    refused("offset_build: X = NULL with Q > 0", build(S.data(), K_obs, nullptr, ldx, Beta.data(), N, Off.data(), N, ldo, Tc, N, K_obs, Q, R));
    refused("offset_build: Q = 0 with R > 1", build(S.data(), K_obs, nullptr, 0, Beta.data(), N, Off.data(), N, ldo, Tc, N, K_obs, 0, R));
    refused("offset_build: R > 1 with shared latents (ldx_r = 0)", build(S.data(), K_obs, X.data(), 0, Beta.data(), N, Off.data(), N, ldo, Tc, N, K_obs, Q, R));
    refused("offset_build: R > 1 with ldo_r too small", build(S.data(), K_obs, X.data(), ldx, Beta.data(), N, Off.data(), N, ldo - 1, Tc, N, K_obs, Q, R));
    refused("offset_build: ldo_t < N", build(S.data(), K_obs, X.data(), ldx, Beta.data(), N, Off.data(), N - 1, ldo, Tc, N, K_obs, Q, R));
    refused("offset_build: ldn < N", build(S.data(), K_obs, X.data(), ldx, Beta.data(), N - 1, Off.data(), N, ldo, Tc, N, K_obs, Q, R));
    refused("offset_build: Tc = 0", build(S.data(), K_obs, X.data(), ldx, Beta.data(), N, Off.data(), N, ldo, 0, N, K_obs, Q, R));
    refused("offset_build: R = 0", build(S.data(), K_obs, X.data(), ldx, Beta.data(), N, Off.data(), N, ldo, Tc, N, K_obs, Q, 0));
    refused("offset_build: Beta = NULL", build(S.data(), K_obs, X.data(), ldx, nullptr, N, Off.data(), N, ldo, Tc, N, K_obs, Q, R));
    refused("offset_build: Off = NULL", build(S.data(), K_obs, X.data(), ldx, Beta.data(), N, nullptr, N, ldo, Tc, N, K_obs, Q, R));

    std::vector<double> carry(R * Q), phi = {0.5, 0.0}, s = {std::sqrt(0.75), 1.0};       // exactly Q entries: a check that read phi[Q] would show
    auto paths = [&](double* x, long ldx_r, int r, long rep0, int tc, int q, const double* ph, const double* sq, double* c, int has) {
        return pgl_latent_prior_paths(x, ldx_r, r, rep0, 0, tc, q, ph, sq, c, has, nullptr, 1, nullptr);
    };
    const double one[2] = {1.0, 0.0}, neg[2] = {-0.1, 0.0}, nan[2] = {std::nan(""), 0.0}, zero[2] = {0.0, 1.0}, big[2] = {1.5, 1.0};
    refused("prior_paths: Q = 0", paths(X.data(), ldx, R, 0, Tc, 0, phi.data(), s.data(), carry.data(), 0));
    refused("prior_paths: Q = 9 (phi and s hold 2 entries)", paths(X.data(), ldx, R, 0, Tc, 9, phi.data(), s.data(), carry.data(), 0));
    refused("prior_paths: R = 0", paths(X.data(), ldx, 0, 0, Tc, Q, phi.data(), s.data(), carry.data(), 0));
    refused("prior_paths: Tc = 0", paths(X.data(), ldx, R, 0, 0, Q, phi.data(), s.data(), carry.data(), 0));
    refused("prior_paths: rep0 < 0", paths(X.data(), ldx, R, -1, Tc, Q, phi.data(), s.data(), carry.data(), 0));
    refused("prior_paths: rep0 + R beyond 2^31", paths(X.data(), ldx, R, (1L << 31) - 2, Tc, Q, phi.data(), s.data(), carry.data(), 0));
    refused("prior_paths: has_carry = 2", paths(X.data(), ldx, R, 0, Tc, Q, phi.data(), s.data(), carry.data(), 2));
    refused("prior_paths: ldx_r < Tc Q", paths(X.data(), ldx - 1, R, 0, Tc, Q, phi.data(), s.data(), carry.data(), 0));
    refused("prior_paths: X = NULL", paths(nullptr, ldx, R, 0, Tc, Q, phi.data(), s.data(), carry.data(), 0));
    refused("prior_paths: carry = NULL", paths(X.data(), ldx, R, 0, Tc, Q, phi.data(), s.data(), nullptr, 0));
    refused("prior_paths: phi = NULL", paths(X.data(), ldx, R, 0, Tc, Q, nullptr, s.data(), carry.data(), 0));
    refused("prior_paths: s = NULL", paths(X.data(), ldx, R, 0, Tc, Q, phi.data(), nullptr, carry.data(), 0));
    refused("prior_paths: phi = 1", paths(X.data(), ldx, R, 0, Tc, Q, one, s.data(), carry.data(), 0));
    refused("prior_paths: phi < 0", paths(X.data(), ldx, R, 0, Tc, Q, neg, s.data(), carry.data(), 0));
    refused("prior_paths: phi is NaN", paths(X.data(), ldx, R, 0, Tc, Q, nan, s.data(), carry.data(), 0));
    refused("prior_paths: s = 0", paths(X.data(), ldx, R, 0, Tc, Q, phi.data(), zero, carry.data(), 0));
    refused("prior_paths: s > 1", paths(X.data(), ldx, R, 0, Tc, Q, phi.data(), big, carry.data(), 0));

    std::printf("%d refusal(s) missing\n", failures);
    return failures ? 1 : 0;
}
