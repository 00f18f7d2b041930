// dgp_prior.h -- the host side of dgp_prior_samples (no HIP in here): the constants the kernel takes by value, formed in double in the order include/dgpmp2_hip.h
// states (tests/prior_oracle.py restates them; the kernel is held against that bit for bit, so every operation below is part of the contract), and the closed form
// of P(t) that the host (for S) and the lanes (for P_k) share.  Needs nothing of the solver: the configuration is read through the handle's first member.
#pragma once
#include <math.h>
#include <stdint.h>
#include "dgp_status.h"

#if defined(__HIPCC__)
#define DGP_PRIOR_HD __host__ __device__ __forceinline__
#else
#define DGP_PRIOR_HD inline
#endif

namespace dgp_prior {

constexpr int kMaxSamples = 1 << 24;      // the sample index shares a counter word with the stream tag
constexpr uint32_t kStreamTag = 0x50u;    // counter word 3 = (kStreamTag << 24) | s: dgp_sample_problems uses 0 and 1 there, dgp_obstacle_maps 0 .. 63 and 0xffffffff

// THE choice of the kernel a launch runs (dgp_prior_samples dispatches on it, dgp_prior_launch_shape reports it): lanes per trajectory from the number of states;
// past 64 states one wavefront walks `blocks` blocks of 64 states, twice
struct LaunchShape { int lpt, blocks; };
inline LaunchShape launch_shape(int n) { return LaunchShape{n <= 16 ? 16 : (n <= 32 ? 32 : 64), (n + 63) / 64}; }

struct PriorConsts {
  double dt, t_end;            // the handle's dt; t_end = (double)(n - 1) * dt
  double ks, kg, ks2;          // K_s, K_g, K_s * K_s
  double cp, cv1, cv2;         // the noise of one interval: position cp * L_c u, velocity cv1 * L_c u + cv2 * L_c u'
  double Lc[9], Qc[9];         // dof x dof, row-major: Q_c = (Q_c_inv)^-1 and its lower Cholesky factor
  double Sinv[36];             // d x d, row-major: (P(t_end) + K_g^2 I)^-1
};

// The coefficients of P(t) = K_s^2 Phi(t) Phi(t)^T + Q(t):  P_pp = i_pp I + q_pp Q_c,  P_pv = i_pv I + q_pv Q_c,  P_vv = ks2 I + q_vv Q_c
struct PCoef { double i_pp, i_pv, q_pp, q_pv, q_vv; };
DGP_PRIOR_HD PCoef p_coef(double ks2, double t) {
#pragma clang fp contract(off)
  const double t2 = t * t;
  const double t3 = t2 * t;
  PCoef c;
  c.i_pp = ks2 * (1.0 + t2);
  c.i_pv = ks2 * t;
  c.q_pp = t3 / 3.0;
  c.q_pv = t2 / 2.0;
  c.q_vv = t;
  return c;
}

// Lower Cholesky factor G of the symmetric N x N matrix A (row-major, lower triangle read): false where a pivot is not positive (NaN included)
inline bool cholesky(const double* A, int N, double* G) {
#pragma clang fp contract(off)
  for (int k = 0; k < N * N; ++k) G[k] = 0.0;
  for (int j = 0; j < N; ++j) {
    double s = A[j * N + j];
    for (int k = 0; k < j; ++k) s = s - G[j * N + k] * G[j * N + k];
    if (!(s > 0.0) || !(s < HUGE_VAL)) return false;
    G[j * N + j] = sqrt(s);
    for (int i = j + 1; i < N; ++i) {
      double r = A[i * N + j];
      for (int k = 0; k < j; ++k) r = r - G[i * N + k] * G[j * N + k];
      G[i * N + j] = r / G[j * N + j];
    }
  }
  return true;
}

// A^-1 = G^-T G^-1 of an SPD matrix: Ginv by forward substitution, then the product, the lower triangle computed and mirrored
inline bool spd_inverse(const double* A, int N, double* Ainv) {
#pragma clang fp contract(off)
  double G[36], W[36];
  if (!cholesky(A, N, G)) return false;
  for (int k = 0; k < N * N; ++k) W[k] = 0.0;
  for (int j = 0; j < N; ++j) {
    W[j * N + j] = 1.0 / G[j * N + j];
    for (int i = j + 1; i < N; ++i) {
      double s = G[i * N + j] * W[j * N + j];
      for (int k = j + 1; k < i; ++k) s = s + G[i * N + k] * W[k * N + j];
      W[i * N + j] = (-s) / G[i * N + i];
    }
  }
  for (int i = 0; i < N; ++i)
    for (int j = 0; j <= i; ++j) {
      double s = W[i * N + i] * W[i * N + j];
      for (int k = i + 1; k < N; ++k) s = s + W[k * N + i] * W[k * N + j];
      Ainv[i * N + j] = Ainv[j * N + i] = s;
    }
  return true;
}

// -> DGP_OK, or DGP_EINVAL with the text set: Q_c_inv not symmetric positive definite (or the matrix S, which is SPD whenever Q_c is)
inline int fill_consts(const DgpConfig& c, PriorConsts& k) {
#pragma clang fp contract(off)
  const int dof = c.dof, d = 2 * dof, n = c.num_states;
  for (int i = 0; i < dof; ++i)
    for (int j = 0; j < i; ++j)
      if (!(c.Q_c_inv[i * dof + j] == c.Q_c_inv[j * dof + i]))
        return dgp_host::fail(DGP_EINVAL, "dgp_prior_samples: Q_c_inv is not symmetric (entries (%d,%d) and (%d,%d) differ): no SPD sampling law", i, j, j, i);
  for (int k2 = 0; k2 < 9; ++k2) k.Lc[k2] = k.Qc[k2] = 0.0;
  if (!spd_inverse(c.Q_c_inv, dof, k.Qc) || !cholesky(k.Qc, dof, k.Lc))
    return dgp_host::fail(DGP_EINVAL, "dgp_prior_samples: Q_c_inv is not symmetric positive definite: it has no inverse Q_c with a Cholesky factor");
  k.dt = c.total_time_sec * 1.0 / (double)(n - 1) * 1.0;      // the handle's dt (plan_layer.py:31)
  k.t_end = (double)(n - 1) * k.dt;
  k.ks = c.K_s; k.kg = c.K_g; k.ks2 = c.K_s * c.K_s;
  const double sdt = sqrt(k.dt), s3 = sqrt(3.0);
  k.cp = (k.dt * sdt) / s3;
  k.cv1 = (s3 / 2.0) * sdt;
  k.cv2 = sdt / 2.0;
  const PCoef pc = p_coef(k.ks2, k.t_end);
  const double kg2 = c.K_g * c.K_g;
  double S[36];
  for (int i = 0; i < dof; ++i)
    for (int j = 0; j < dof; ++j) {
      const double q = k.Qc[i * dof + j], e = i == j ? 1.0 : 0.0;
      S[i * d + j] = (pc.i_pp + kg2) * e + pc.q_pp * q;
      S[i * d + dof + j] = S[(dof + i) * d + j] = pc.i_pv * e + pc.q_pv * q;
      S[(dof + i) * d + dof + j] = (k.ks2 + kg2) * e + pc.q_vv * q;
    }
  for (int k2 = 0; k2 < 36; ++k2) k.Sinv[k2] = 0.0;
  if (!spd_inverse(S, d, k.Sinv)) return dgp_host::fail(DGP_EINVAL, "dgp_prior_samples: the goal-observation covariance S is not positive definite (K_s, K_g, Q_c_inv)");
  return DGP_OK;
}

}  // namespace dgp_prior
