// statespace.hpp — the small dense algebra of the state-space (Kalman) form of a one-dimensional Matern GP: the model matrices, the
// elements of the two associative scans (Sarkka & Garcia-Fernandez 2021) and their combination rules, for state dimension D = 2
// (Matern-3/2) or 3 (Matern-5/2).  Everything is fp64, lives in registers (every loop has compile-time bounds) and compiles for the host
// as well, so that the rules can be exercised without a device.  statespace.hip: the kernels; statespace_api.hip: the C-ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace svgp {
namespace ss {

#define SS_HD __host__ __device__ __forceinline__

constexpr int kTile = 64;   // points per workgroup at every level of a scan: one wavefront, one element per lane

template <int D> struct Dim { static constexpr int TRI = D * (D + 1) / 2; };
// index of (i, j) in the stored upper triangle, rows ascending
template <int D> SS_HD constexpr int tri(int i, int j) { return i <= j ? i * D - i * (i - 1) / 2 + (j - i) : j * D - j * (j - 1) / 2 + (i - j); }

struct Model {   // one parameter set
  double variance, lam;   // lam = sqrt(2 nu) inv_lengthscale
};

template <int D> SS_HD void pinf(const Model& m, double P[D][D]) {
  const double l2 = m.lam * m.lam;
  if constexpr (D == 2) {
    P[0][0] = m.variance; P[0][1] = 0; P[1][0] = 0; P[1][1] = l2 * m.variance;
  } else {
    const double k = m.variance * l2 / 3.0;
    P[0][0] = m.variance; P[0][1] = 0; P[0][2] = -k;
    P[1][0] = 0; P[1][1] = k; P[1][2] = 0;
    P[2][0] = -k; P[2][1] = 0; P[2][2] = l2 * l2 * m.variance;
  }
}

// A(dt) = exp(-lam dt) sum_{p < D} N^p dt^p / p!,  N = F + lam I (nilpotent);  Q(dt) = Pinf - A Pinf A'.  dt = 0: A = I, Q = 0 exactly
template <int D> SS_HD void transition(const Model& m, double dt, double A[D][D], double Q[D][D]) {
  const double l = m.lam, e = exp(-l * dt), x = l * dt;
  if constexpr (D == 2) {
    A[0][0] = e * (1.0 + x); A[0][1] = e * dt;
    A[1][0] = -e * l * x;    A[1][1] = e * (1.0 - x);
  } else {
    // N = [[l, 1, 0], [0, l, 1], [-l^3, -3 l^2, -2 l]],  N^2 = [[l^2, 2 l, 1], [-l^3, -2 l^2, -l], [l^4, 2 l^3, l^2]]
    const double h = 0.5 * dt * dt, l2 = l * l;
    A[0][0] = e * (1.0 + x + h * l2);      A[0][1] = e * (dt + 2.0 * h * l);          A[0][2] = e * h;
    A[1][0] = -e * h * l2 * l;             A[1][1] = e * (1.0 + x - 2.0 * h * l2);    A[1][2] = e * (dt - h * l);
    A[2][0] = e * (h * l2 * l2 - x * l2);  A[2][1] = e * (2.0 * h * l2 * l - 3.0 * x * l);  A[2][2] = e * (1.0 - 2.0 * x + h * l2);
  }
  double P[D][D], AP[D][D];
  pinf<D>(m, P);
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = 0; j < D; ++j) {
      double s = 0;
#pragma unroll
      for (int k = 0; k < D; ++k) s += A[i][k] * P[k][j];
      AP[i][j] = s;
    }
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = i; j < D; ++j) {
      double s = 0;
#pragma unroll
      for (int k = 0; k < D; ++k) s += AP[i][k] * A[j][k];
      Q[i][j] = Q[j][i] = P[i][j] - s;
    }
}

template <int D> SS_HD void matmul(const double X[D][D], const double Y[D][D], double Z[D][D]) {
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = 0; j < D; ++j) {
      double s = 0;
#pragma unroll
      for (int k = 0; k < D; ++k) s += X[i][k] * Y[k][j];
      Z[i][j] = s;
    }
}
template <int D> SS_HD void matmul_nt(const double X[D][D], const double Y[D][D], double Z[D][D]) {   // X Y'
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = 0; j < D; ++j) {
      double s = 0;
#pragma unroll
      for (int k = 0; k < D; ++k) s += X[i][k] * Y[j][k];
      Z[i][j] = s;
    }
}
template <int D> SS_HD void matmul_tn(const double X[D][D], const double Y[D][D], double Z[D][D]) {   // X' Y
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = 0; j < D; ++j) {
      double s = 0;
#pragma unroll
      for (int k = 0; k < D; ++k) s += X[k][i] * Y[k][j];
      Z[i][j] = s;
    }
}
template <int D> SS_HD void unpack(const double* t, double X[D][D]) {
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = 0; j < D; ++j) X[i][j] = t[tri<D>(i, j)];
}
// the stored triangle of a product that is symmetric in exact arithmetic: the mean of its two halves
template <int D> SS_HD void pack_sym(const double X[D][D], double* t) {
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = i; j < D; ++j) t[tri<D>(i, j)] = 0.5 * (X[i][j] + X[j][i]);
}

// (I + X)^-1 in closed form (adjugate / determinant).  For X = C J with C, J symmetric positive semi-definite the determinant is >= 1
template <int D> SS_HD void inv_i_plus(const double X[D][D], double M[D][D]) {
  if constexpr (D == 2) {
    const double a = 1.0 + X[0][0], b = X[0][1], c = X[1][0], d = 1.0 + X[1][1];
    const double r = 1.0 / (a * d - b * c);
    M[0][0] = d * r; M[0][1] = -b * r; M[1][0] = -c * r; M[1][1] = a * r;
  } else {
    const double a = 1.0 + X[0][0], b = X[0][1], c = X[0][2], d = X[1][0], e = 1.0 + X[1][1], f = X[1][2], g = X[2][0], h = X[2][1],
                 i = 1.0 + X[2][2];
    const double c00 = e * i - f * h, c01 = f * g - d * i, c02 = d * h - e * g;
    const double r = 1.0 / (a * c00 + b * c01 + c * c02);
    M[0][0] = c00 * r; M[0][1] = (c * h - b * i) * r; M[0][2] = (b * f - c * e) * r;
    M[1][0] = c01 * r; M[1][1] = (a * i - c * g) * r; M[1][2] = (c * d - a * f) * r;
    M[2][0] = c02 * r; M[2][1] = (b * g - a * h) * r; M[2][2] = (a * e - b * d) * r;
  }
}

// X <- X S^-1 for a symmetric positive definite S, by its unpivoted L D L' factor in registers
template <int D> SS_HD void solve_right_spd(const double S[D][D], double X[D][D]) {
  double L[D][D], dg[D];
#pragma unroll
  for (int j = 0; j < D; ++j) {
    double s = S[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) s -= L[j][k] * L[j][k] * dg[k];
    dg[j] = s;
    const double inv = 1.0 / s;
#pragma unroll
    for (int i = j + 1; i < D; ++i) {
      double u = S[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) u -= L[i][k] * L[j][k] * dg[k];
      L[i][j] = u * inv;
    }
  }
#pragma unroll
  for (int r = 0; r < D; ++r) {   // row r of X: x S^-1 = ((x L^-T) D^-1) L^-1
#pragma unroll
    for (int j = 0; j < D; ++j) {
#pragma unroll
      for (int k = 0; k < j; ++k) X[r][j] -= X[r][k] * L[j][k];
    }
#pragma unroll
    for (int j = 0; j < D; ++j) X[r][j] /= dg[j];
#pragma unroll
    for (int j = D - 1; j >= 0; --j) {
#pragma unroll
      for (int k = j + 1; k < D; ++k) X[r][j] -= X[r][k] * L[k][j];
    }
  }
}

// ---- the filter's scan: element (A, b, C, eta, J), C and J symmetric (stored triangles) ------------------------------------------
template <int D> struct FiltElem {
  static constexpr int TRI = Dim<D>::TRI;
  static constexpr int oA = 0, ob = D * D, oC = ob + D, oe = oC + TRI, oJ = oe + D, NV = oJ + TRI;
  double v[NV];

  SS_HD static FiltElem identity() {
    FiltElem e;
#pragma unroll
    for (int i = 0; i < NV; ++i) e.v[i] = 0.0;
#pragma unroll
    for (int i = 0; i < D; ++i) e.v[oA + i * D + i] = 1.0;
    return e;
  }

  // the element of point k: the transition over dt = t_k - t_{k-1} and the observation (dl = y_k - mean, noise variance r; r < 0: no
  // observation).  first: the ordinary update of (0, Pinf)
  SS_HD static FiltElem build(const Model& m, bool first, double dt, double dl, double r) {
    FiltElem e;
    double F[D][D], Q[D][D];
    if (first) {
      pinf<D>(m, Q);
#pragma unroll
      for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j < D; ++j) F[i][j] = 0.0;
    } else {
      transition<D>(m, dt, F, Q);
    }
    const bool obs = r >= 0.0;
    const double is = obs ? 1.0 / (Q[0][0] + r) : 0.0;
    double K[D];
#pragma unroll
    for (int i = 0; i < D; ++i) K[i] = Q[i][0] * is;
#pragma unroll
    for (int i = 0; i < D; ++i) {
#pragma unroll
      for (int j = 0; j < D; ++j) e.v[oA + i * D + j] = F[i][j] - K[i] * F[0][j];
      e.v[ob + i] = K[i] * dl;
      e.v[oe + i] = F[0][i] * dl * is;
    }
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = i; j < D; ++j) {
        e.v[oC + tri<D>(i, j)] = Q[i][j] - K[i] * Q[0][j];
        e.v[oJ + tri<D>(i, j)] = F[0][i] * F[0][j] * is;
      }
    return e;
  }

  // x before y
  SS_HD static FiltElem combine(const FiltElem& x, const FiltElem& y) {
    double Ci[D][D], Jj[D][D], Ai[D][D], Aj[D][D], X[D][D], M[D][D], AjM[D][D], T1[D][D], T2[D][D];
    unpack<D>(x.v + oC, Ci);
    unpack<D>(y.v + oJ, Jj);
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = 0; j < D; ++j) { Ai[i][j] = x.v[oA + i * D + j]; Aj[i][j] = y.v[oA + i * D + j]; }
    matmul<D>(Ci, Jj, X);
    inv_i_plus<D>(X, M);          // M = (I + C_i J_j)^-1;  (I + J_j C_i)^-1 = M'
    matmul<D>(Aj, M, AjM);
    FiltElem o;
    matmul<D>(AjM, Ai, T1);
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = 0; j < D; ++j) o.v[oA + i * D + j] = T1[i][j];
    double u[D], w[D];
#pragma unroll
    for (int i = 0; i < D; ++i) {   // u = b_i + C_i eta_j,  w = eta_j - J_j b_i
      double s = x.v[ob + i], q = y.v[oe + i];
#pragma unroll
      for (int k = 0; k < D; ++k) { s += Ci[i][k] * y.v[oe + k]; q -= Jj[i][k] * x.v[ob + k]; }
      u[i] = s;
      w[i] = q;
    }
#pragma unroll
    for (int i = 0; i < D; ++i) {
      double s = y.v[ob + i];
#pragma unroll
      for (int k = 0; k < D; ++k) s += AjM[i][k] * u[k];
      o.v[ob + i] = s;
    }
    matmul<D>(AjM, Ci, T1);
    matmul_nt<D>(T1, Aj, T2);       // A_j M C_i A_j'
    pack_sym<D>(T2, o.v + oC);
#pragma unroll
    for (int i = 0; i < TRI; ++i) o.v[oC + i] += y.v[oC + i];
    matmul<D>(M, Ai, T1);           // W' = M A_i,  W = A_i' M'
    double mw[D];
#pragma unroll
    for (int i = 0; i < D; ++i) {   // M' w
      double s = 0;
#pragma unroll
      for (int k = 0; k < D; ++k) s += M[k][i] * w[k];
      mw[i] = s;
    }
#pragma unroll
    for (int i = 0; i < D; ++i) {
      double s = x.v[oe + i];
#pragma unroll
      for (int k = 0; k < D; ++k) s += Ai[k][i] * mw[k];
      o.v[oe + i] = s;
    }
    matmul<D>(Jj, T1, T2);          // J = A_i' M' J_j A_i + J_i with M' J_j = J_j M (push-through): T2 = J_j M A_i
    matmul_tn<D>(Ai, T2, T1);
    pack_sym<D>(T1, o.v + oJ);
#pragma unroll
    for (int i = 0; i < TRI; ++i) o.v[oJ + i] += x.v[oJ + i];
    return o;
  }
};

// ---- the smoother's scan (in reverse): element (E, g, L), L symmetric ------------------------------------------------------------
template <int D> struct SmoothElem {
  static constexpr int TRI = Dim<D>::TRI;
  static constexpr int oE = 0, og = D * D, oL = og + D, NV = oL + TRI;
  double v[NV];

  SS_HD static SmoothElem identity() {
    SmoothElem e;
#pragma unroll
    for (int i = 0; i < NV; ++i) e.v[i] = 0.0;
#pragma unroll
    for (int i = 0; i < D; ++i) e.v[oE + i * D + i] = 1.0;
    return e;
  }

  // the element of point k from its filtered moments (mk, Pk as a stored triangle) and the transition over dt = t_{k+1} - t_k.
  // last: (0, m_n, P_n)
  SS_HD static SmoothElem build(const Model& m, bool last, double dt, const double* mk, const double* Pk) {
    SmoothElem e;
    if (last) {
#pragma unroll
      for (int i = 0; i < D * D; ++i) e.v[oE + i] = 0.0;
#pragma unroll
      for (int i = 0; i < D; ++i) e.v[og + i] = mk[i];
#pragma unroll
      for (int i = 0; i < TRI; ++i) e.v[oL + i] = Pk[i];
      return e;
    }
    double F[D][D], Q[D][D], P[D][D], FP[D][D], S[D][D], E[D][D], T1[D][D];
    transition<D>(m, dt, F, Q);
    unpack<D>(Pk, P);
    matmul<D>(F, P, FP);
    matmul_nt<D>(FP, F, S);
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = 0; j < D; ++j) E[i][j] = FP[j][i];   // P F'
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = i; j < D; ++j) S[i][j] = S[j][i] = S[i][j] + Q[i][j];   // one triangle: exactly symmetric
    solve_right_spd<D>(S, E);      // E = P F' (F P F' + Q)^-1
    double fm[D];
#pragma unroll
    for (int i = 0; i < D; ++i) {
      double s = 0;
#pragma unroll
      for (int k = 0; k < D; ++k) s += F[i][k] * mk[k];
      fm[i] = s;
    }
    matmul<D>(E, FP, T1);          // E F P
#pragma unroll
    for (int i = 0; i < D; ++i) {
      double s = mk[i];
#pragma unroll
      for (int k = 0; k < D; ++k) s -= E[i][k] * fm[k];
      e.v[og + i] = s;
#pragma unroll
      for (int j = 0; j < D; ++j) e.v[oE + i * D + j] = E[i][j];
    }
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = i; j < D; ++j) e.v[oL + tri<D>(i, j)] = P[i][j] - 0.5 * (T1[i][j] + T1[j][i]);
    return e;
  }

  // x before y in the scan's order.  The scan runs from the last point to the first, so y holds the earlier points (the rule's i) and
  // x the later ones (its j): E = E_y E_x, g = E_y g_x + g_y, L = E_y L_x E_y' + L_y
  SS_HD static SmoothElem combine(const SmoothElem& x, const SmoothElem& y) {
    double Ei[D][D], Ej[D][D], Lj[D][D], T1[D][D], T2[D][D];
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = 0; j < D; ++j) { Ei[i][j] = y.v[oE + i * D + j]; Ej[i][j] = x.v[oE + i * D + j]; }
    unpack<D>(x.v + oL, Lj);
    SmoothElem o;
    matmul<D>(Ei, Ej, T1);
#pragma unroll
    for (int i = 0; i < D; ++i) {
      double s = y.v[og + i];
#pragma unroll
      for (int k = 0; k < D; ++k) s += Ei[i][k] * x.v[og + k];
      o.v[og + i] = s;
#pragma unroll
      for (int j = 0; j < D; ++j) o.v[oE + i * D + j] = T1[i][j];
    }
    matmul<D>(Ei, Lj, T1);
    matmul_nt<D>(T1, Ei, T2);
    pack_sym<D>(T2, o.v + oL);
#pragma unroll
    for (int i = 0; i < TRI; ++i) o.v[oL + i] += y.v[oL + i];
    return o;
  }
};

// the one-step prediction at point k from the filtered moments of point k - 1 (first: the prior): its first mean entry and P^-_11
template <int D> SS_HD void predict_obs(const Model& m, bool first, double dt, const double* mp, const double* Pp, double* mean, double* var) {
  if (first) { *mean = 0.0; *var = m.variance; return; }
  double F[D][D], Q[D][D], P[D][D];
  transition<D>(m, dt, F, Q);
  unpack<D>(Pp, P);
  double mu = 0, s = Q[0][0];
#pragma unroll
  for (int i = 0; i < D; ++i) {
    mu += F[0][i] * mp[i];
#pragma unroll
    for (int j = 0; j < D; ++j) s += F[0][i] * P[i][j] * F[0][j];
  }
  *mean = mu;
  *var = s;
}

// ---- the sampler's scans: affine maps x -> A x + c over SC right-hand sides at once ---------------------------------------------------
// Joint posterior paths by Matheron's rule in state-space form (the Durbin-Koopman simulation smoother) are three recursions of one
// shape: the prior path x_k = A_k x_{k-1} + Lq_k z_k, the filter's means m_k = Abar_k m_{k-1} + K_k rho_k of the residual rho, and the
// smoother's means mhat_k = E_k mhat_{k+1} + (I - E_k A_{k+1}) m_k.  Their matrices do not depend on the draws (the gains come from the
// filtered covariances of one ordinary filter scan), so a chunk of SC samples shares A and carries c as D x SC, sample fastest.

// the lower factor Lq of a symmetric positive SEMI-definite S = Lq Lq', by an unpivoted L D L' in registers.  A pivot that is not > 0
// (a singular or indefinite-by-rounding S, NaN included) is replaced by 0 together with its column: dt = 0 gives Lq = 0, never a NaN
template <int D> SS_HD void psd_factor(const double S[D][D], double Lq[D][D]) {
  double L[D][D], dg[D];
#pragma unroll
  for (int j = 0; j < D; ++j) {
    double s = S[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) s -= L[j][k] * L[j][k] * dg[k];
    const bool ok = s > 0.0;
    dg[j] = ok ? s : 0.0;
    const double inv = ok ? 1.0 / s : 0.0, rt = ok ? sqrt(s) : 0.0;
#pragma unroll
    for (int i = 0; i < j; ++i) Lq[i][j] = 0.0;
    Lq[j][j] = rt;
#pragma unroll
    for (int i = j + 1; i < D; ++i) {
      double u = S[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) u -= L[i][k] * L[j][k] * dg[k];
      L[i][j] = u * inv;
      Lq[i][j] = L[i][j] * rt;
    }
  }
}

template <int D, int SC> struct AffineElem {
  static constexpr int TRI = Dim<D>::TRI;
  static constexpr int oA = 0, oc = D * D, NV = oc + D * SC;   // c[i][s] at oc + i * SC + s
  double v[NV];

  SS_HD static AffineElem identity() {
    AffineElem e;
#pragma unroll
    for (int i = 0; i < NV; ++i) e.v[i] = 0.0;
#pragma unroll
    for (int i = 0; i < D; ++i) e.v[oA + i * D + i] = 1.0;
    return e;
  }

  // x before y (x is applied first): (A_y A_x, A_y c_x + c_y)
  SS_HD static AffineElem combine(const AffineElem& x, const AffineElem& y) {
    AffineElem o;
#pragma unroll
    for (int i = 0; i < D; ++i) {
#pragma unroll
      for (int j = 0; j < D; ++j) {
        double s = 0;
#pragma unroll
        for (int k = 0; k < D; ++k) s += y.v[oA + i * D + k] * x.v[oA + k * D + j];
        o.v[oA + i * D + j] = s;
      }
#pragma unroll
      for (int q = 0; q < SC; ++q) {
        double s = y.v[oc + i * SC + q];
#pragma unroll
        for (int k = 0; k < D; ++k) s += y.v[oA + i * D + k] * x.v[oc + k * SC + q];
        o.v[oc + i * SC + q] = s;
      }
    }
    return o;
  }

  SS_HD void set(const double A[D][D]) {
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = 0; j < D; ++j) v[oA + i * D + j] = A[i][j];
  }

  // the prior path at point k: x_k = A(dt) x_{k-1} + Lq z_k, Lq Lq' = Q(dt); first: x_0 = chol(Pinf) z_0.  z: [D][SC] standard normals
  SS_HD static AffineElem build_prior(const Model& m, bool first, double dt, const double* z) {
    AffineElem e;
    double F[D][D], Q[D][D], Lq[D][D];
    if (first) {
      pinf<D>(m, Q);
#pragma unroll
      for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j < D; ++j) F[i][j] = 0.0;
    } else {
      transition<D>(m, dt, F, Q);
    }
    psd_factor<D>(Q, Lq);
    e.set(F);
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int q = 0; q < SC; ++q) {
        double s = 0;
#pragma unroll
        for (int k = 0; k <= i; ++k) s += Lq[i][k] * z[k * SC + q];
        e.v[oc + i * SC + q] = s;
      }
    return e;
  }

  // the filter's mean at point k for the residual rho_k = dl - ft - sqrt(r) eps (ft: the prior path's first entry, [SC]; eps: [SC]),
  // fused in: m_k = (I - K H) A m_{k-1} + K rho_k, K = P^- H' / (P^-_11 + r), P^- = A P_{k-1} A' + Q from the filtered covariance Pp of
  // point k - 1 (a stored triangle).  r < 0: no observation, K = 0.  first: the update of (0, Pinf)
  SS_HD static AffineElem build_filter(const Model& m, bool first, double dt, const double* Pp, double r, double dl, const double* ft,
                                       const double* eps) {
    AffineElem e;
    double F[D][D], Q[D][D];
    if (first) {
      pinf<D>(m, Q);
#pragma unroll
      for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j < D; ++j) F[i][j] = 0.0;
    } else {
      double P[D][D], FP[D][D], S[D][D];
      transition<D>(m, dt, F, Q);
      unpack<D>(Pp, P);
      matmul<D>(F, P, FP);
      matmul_nt<D>(FP, F, S);
#pragma unroll
      for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = i; j < D; ++j) Q[i][j] = Q[j][i] = Q[i][j] + 0.5 * (S[i][j] + S[j][i]);
    }
    const bool obs = r >= 0.0;
    const double is = obs ? 1.0 / (Q[0][0] + r) : 0.0, sr = obs ? sqrt(r) : 0.0;
    double K[D];
#pragma unroll
    for (int i = 0; i < D; ++i) K[i] = Q[i][0] * is;
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = 0; j < D; ++j) e.v[oA + i * D + j] = F[i][j] - K[i] * F[0][j];
#pragma unroll
    for (int q = 0; q < SC; ++q) {
      const double rho = dl - ft[q] - sr * eps[q];
#pragma unroll
      for (int i = 0; i < D; ++i) e.v[oc + i * SC + q] = K[i] * rho;
    }
    return e;
  }

  // the smoother's mean at point k, scanned from the last point to the first: mhat_k = E mhat_{k+1} + (m_k - E A m_k) with the gain
  // E = P_k A' (A P_k A' + Q)^-1 of SmoothElem::build, dt = t_{k+1} - t_k.  mk: the filtered means [D][SC].  last: mhat = m
  SS_HD static AffineElem build_smooth(const Model& m, bool last, double dt, const double* Pk, const double* mk) {
    AffineElem e;
    if (last) {
#pragma unroll
      for (int i = 0; i < D * D; ++i) e.v[oA + i] = 0.0;
#pragma unroll
      for (int i = 0; i < D * SC; ++i) e.v[oc + i] = mk[i];
      return e;
    }
    double F[D][D], Q[D][D], P[D][D], FP[D][D], S[D][D], E[D][D];
    transition<D>(m, dt, F, Q);
    unpack<D>(Pk, P);
    matmul<D>(F, P, FP);
    matmul_nt<D>(FP, F, S);
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = 0; j < D; ++j) E[i][j] = FP[j][i];   // P F'
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = i; j < D; ++j) S[i][j] = S[j][i] = S[i][j] + Q[i][j];
    solve_right_spd<D>(S, E);
    e.set(E);
#pragma unroll
    for (int q = 0; q < SC; ++q) {
      double fm[D];
#pragma unroll
      for (int i = 0; i < D; ++i) {
        double s = 0;
#pragma unroll
        for (int k = 0; k < D; ++k) s += F[i][k] * mk[k * SC + q];
        fm[i] = s;
      }
#pragma unroll
      for (int i = 0; i < D; ++i) {
        double s = mk[i * SC + q];
#pragma unroll
        for (int k = 0; k < D; ++k) s -= E[i][k] * fm[k];
        e.v[oc + i * SC + q] = s;
      }
    }
    return e;
  }
};

}  // namespace ss
}  // namespace svgp
