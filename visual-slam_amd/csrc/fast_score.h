// FAST-9/16 arc network on the raw circle pixels, shared by k_fast (device, 16-bit VOP2 min / max by inline asm) and the CPU test
// of the network (host, std::min / std::max).
//
// With d_k = v - p_k (v the centre, p_k the 16 circle pixels in OpenCV order) the one-sided scores are
//   darker arc:   max over the 16 arcs of min over the arc of d  =  v - (min over arcs of max over the arc of p)
//   brighter arc: max over the 16 arcs of min over the arc of -d = (max over arcs of min over the arc of p) - v
// because min_k (v - p_k) = v - max_k p_k.  Both are fast_arc_extreme below with its two operations exchanged, followed by ONE
// subtraction; no per-pixel differences are formed.  The inner extreme over each circular 9-arc uses block suffix / prefix
// extremes (van Herk / Gil-Werman) over the circle unrolled to 24 entries q[i] = p[i & 15], blocks q[0..8], q[9..17], q[18..23]:
// arc 0 and arc 9 are whole blocks, arc i in 1..8 is suffix(block 0, from i) with prefix(block 1, to i + 8), arc i in 10..15 is
// suffix(block 1, from i) with prefix(block 2, to i + 8).  42 inner operations + 15 for the outer reduction, against 80 for the
// direct three-by-three network.
#pragma once

#if defined(__HIPCC__) || defined(__HIP__)
#define FAST_HD __host__ __device__ __forceinline__
#else
#define FAST_HD inline
#endif

// in(p[0..15]) -> out over the 16 circular arcs of 9 consecutive pixels of (in over the arc)
template <class In, class Out>
FAST_HD int fast_arc_extreme(const int p[16], In in, Out out) {
    // block 0 = p[0..8]: suffixes s0[i] = in(p[i..8])
    int s0[9];
    s0[8] = p[8];
#pragma unroll
    for (int i = 7; i >= 0; i--) s0[i] = in(p[i], s0[i + 1]);
    // block 1 = p[9..15], p[0], p[1]: prefixes a1[j] = in(q[9..9 + j]), suffixes b1[i] = in(q[9 + i..17])
    int a1[9], b1[9];
    a1[0] = p[9];
#pragma unroll
    for (int j = 1; j < 9; j++) a1[j] = in(a1[j - 1], p[(9 + j) & 15]);
    b1[8] = p[1];
#pragma unroll
    for (int i = 7; i >= 1; i--) b1[i] = in(p[(9 + i) & 15], b1[i + 1]);
    // block 2 = p[2..7]: prefixes a2[j] = in(q[18..18 + j])
    int a2[6];
    a2[0] = p[2];
#pragma unroll
    for (int j = 1; j < 6; j++) a2[j] = in(a2[j - 1], p[2 + j]);
    int r = out(s0[0], a1[8]);  // arcs 0 and 9
#pragma unroll
    for (int i = 1; i < 9; i++) r = out(r, in(s0[i], a1[i - 1]));  // arc i = q[i..8] + q[9..i + 8]
#pragma unroll
    for (int i = 10; i < 16; i++) r = out(r, in(b1[i - 9], a2[i - 10]));  // arc i = q[i..17] + q[18..i + 8]
    return r;
}
