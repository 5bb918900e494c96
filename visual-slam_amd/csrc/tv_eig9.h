// tv_eig9.h -- the 9x9 smallest-eigenvector solver of the two-view refits, shared by k_tv_finish (twoview_kernels.hip: 8-point
// normal matrix) and k_h_finish (twoview_h.hip: homography DLT normal matrix).  Device only; moved here verbatim.
#pragma once

// Smallest eigenvector of the 9x9 normal matrix of a refit on ONE wavefront (rounds 1 - 3: thread 0 alone, LDL^T + at most 16 steps of
// inverse iteration - 16 k cycles per call, 46 % of this kernel, and with an eigenvalue ratio of 0.5 between the two smallest
// eigenvalues 16 steps leave an error of 1.5e-5: the iteration ran into its cap on every pair of the benchmark).  Here the matrix is
// inverted explicitly and the inverse is squared ten times: (M^-1)^(2^10) has the wanted vector as its dominant eigenvector with
// the eigenvalue ratio raised to the 1024th power (0.99 -> 3e-5, 0.9 -> 1e-47).  Both steps work on the 45 entries of the packed upper
// triangle, one per lane:
//   * inverse by the symmetric sweep operator (sweep k: M[k][k] -> -1/d, M[i][k] -> M[i][k]/d, M[i][j] -> M[i][j] - M[i][k] M[k][j]/d;
//     all nine sweeps give -M^-1 and every intermediate matrix is symmetric), on M / trace + 1e-15 I, pivots clamped at 1e-17;
//   * B <- (B / trace B)^2, nine products per lane out of LDS.
// sN: the 45 packed sums (p <= q, row-major) in LDS; sM: 48 doubles of LDS scratch; x[9] in LDS: previous estimate in (its orientation
// is kept), eigenvector out.  Lanes 0..63 of one wavefront, convergent; returns false (x untouched) when the arithmetic broke down.
__device__ __forceinline__ int tv_pk(int p, int q) { return p <= q ? p * 9 - (p * (p - 1)) / 2 + (q - p) : q * 9 - (q * (q - 1)) / 2 + (p - q); }
__device__ __forceinline__ void tv_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
__device__ bool wave_smallest_eigvec9(const double* sN, double* sM, double* x, int lane) {
    int p = 0, q = lane < 45 ? lane : 0;
    while (q >= 9 - p) { q -= 9 - p; p++; }  // packed index -> (p, p + q)
    q += p;
    const bool on = lane < 45;
    double tr = 0.0;
#pragma unroll
    for (int k = 0; k < 9; k++) tr += sN[tv_pk(k, k)];
    if (!(tr > 0.0)) return false;  // (wave-uniform: every lane read the same nine values)
    const double itr = 1.0 / tr;
    if (on) sM[lane] = sN[lane] * itr + (p == q ? 1e-15 : 0.0);
    tv_wave_sync();
    for (int k = 0; k < 9; k++) {  // sweep k
        const double d = fmax(sM[tv_pk(k, k)], 1e-17), id = 1.0 / d;
        const double a = sM[tv_pk(p, k)], b = sM[tv_pk(k, q)], c = sM[lane < 45 ? lane : 0];
        const double nv = p == k && q == k ? -id : p == k ? b * id : q == k ? a * id : c - a * b * id;
        tv_wave_sync();
        if (on) sM[lane] = nv;
        tv_wave_sync();
    }
    // sM = -(M^-1); its square is the square of M^-1
    for (int it = 0; it < 10; it++) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < 9; k++) t += sM[tv_pk(k, k)];
        const double sc = 1.0 / t;  // (trace of a definite matrix: never 0; negative in the first round, squared away)
        // After a round the matrix is (previous / trace)^2: its trace is the sum of the squared normalised eigenvalues, 1 - 2 mu2 / mu1 to first
        // order.  Within 1e-13 of 1 the second direction's share of every column is below 5e-14 and further rounds change nothing that the
        // 1e-4 comparison with the oracle - or this scheme's own 1e-13 distance from eigh - could see: typical normal matrices get there
        // in 3 - 5 rounds, ill-separated ones still take all ten (wave-uniform: every lane read the same nine values).
        // (A/B against the fixed ten rounds: two-view stage 0.385 - 0.389 against 0.387 - 0.392 ms, profiles/r04_ab_tv_bound.txt)
        if (it > 0 && fabs(1.0 - t) < 1e-13) break;
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < 9; k++) acc += sM[tv_pk(p, k)] * sM[tv_pk(k, q)];
        acc *= sc * sc;
        tv_wave_sync();
        if (on) sM[lane] = acc;
        tv_wave_sync();
    }
    // the column with the largest diagonal entry, normalised, oriented like the previous estimate
    int jb = 0;
    double best = sM[tv_pk(0, 0)];
#pragma unroll
    for (int k = 1; k < 9; k++) { const double v = sM[tv_pk(k, k)]; if (v > best) { best = v; jb = k; } }
    double nn = 0.0, dot = 0.0;
#pragma unroll
    for (int k = 0; k < 9; k++) { const double v = sM[tv_pk(k, jb)]; nn += v * v; dot += v * x[k]; }
    if (!(nn > 0.0) || !(nn < 1e300)) return false;  // NaN / overflow somewhere (wave-uniform)
    const double sgn = (dot < 0 ? -1.0 : 1.0) / sqrt(nn);
    const double mine = lane < 9 ? sM[tv_pk(lane, jb)] * sgn : 0.0;
    tv_wave_sync();
    if (lane < 9) x[lane] = mine;
    tv_wave_sync();
    return true;
}
