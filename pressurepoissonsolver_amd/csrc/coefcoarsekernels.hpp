// The sub-patch coarse solve of the variable-coefficient path (te_gmg_set_coef_coarse): a one-patch level of
// n^D cells is the same grid as a uniform tree of (n / s)^D patches of s^D cells. These kernels carry vectors between the two
// layouts; everything that computes is the path's own (coefkernels.hpp), run by an auxiliary solver on the split tree.
//
// origin[q][3]: the cell offsets (x, y, z) of auxiliary patch q inside the big patch, multiples of s; built on the host from the
// auxiliary hierarchy's own level-0 starts (gmg_coefcoarse.hip) -- no patch order is assumed. s, n and every offset are even, so an
// x-pair of cells is 16-byte aligned on both sides: the cell blocks move as double2. Cell c of a patch of m cells per axis sits at
// x + m (y + m z); a face vector holds per patch LO_a (a = 0..D-1, a cell block each), then HI_a (m^(D-1) values, the other axes in
// order).
//
//   k_cc_cells<MERGE>      MERGE = false: aux = split(big) for up to two vectors in one launch (f and u; sigma alone);
//                          MERGE = true:  big = merge(aux), one vector
//   k_cc_split_faces       aux's LO_a = the matching block of big's LO_a; aux's HI_a = big's LO_a plane at offset + s, or big's HI_a
//                          on the patch's upper face: the two copies of a shared face are equal by construction
// At most n^D doubles per vector: launch-bound, one flat grid, nothing tuned.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace te
{
struct CoefCoarseGeom {
	int32_t        D, n, s, Q; // dimension, cells per axis of the big patch and of an auxiliary patch, auxiliary patches
	const int32_t *origin;     // [Q][3]
};

// pair j of auxiliary patch q -> the pair's index in the big patch (both in double2 units)
__device__ __forceinline__ size_t ccBigPair(const CoefCoarseGeom &G, int q, int j)
{
	const int h = G.s / 2, x2 = j % h, y = (j / h) % G.s, z = j / (h * G.s); // (2D: z = 0)
	const int32_t *o = G.origin + (size_t) q * 3;
	return ((size_t) (o[0] / 2 + x2)) + (size_t) (G.n / 2) * ((size_t) (o[1] + y) + (size_t) G.n * (size_t) (o[2] + z));
}

template <bool MERGE>
__global__ __launch_bounds__(256) void k_cc_cells(CoefCoarseGeom G, double2 *__restrict__ big_a, double2 *__restrict__ aux_a,
                                                  const double2 *__restrict__ big_b, double2 *__restrict__ aux_b)
{
	const int    sc2   = (G.D == 3 ? G.s * G.s * G.s : G.s * G.s) / 2; // pairs per auxiliary patch
	const size_t total = (size_t) G.Q * sc2;
	for (size_t idx = (size_t) blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t) gridDim.x * blockDim.x) {
		const int    q = (int) (idx / sc2), j = (int) (idx % sc2);
		const size_t b = ccBigPair(G, q, j);
		if (MERGE) {
			big_a[b] = aux_a[idx];
		} else {
			aux_a[idx] = big_a[b];
			if (big_b) aux_b[idx] = big_b[b];
		}
	}
}

__global__ __launch_bounds__(256) void k_cc_split_faces(CoefCoarseGeom G, const double *__restrict__ big, double *__restrict__ aux)
{
	const int    D = G.D, n = G.n, s = G.s;
	const int    sc = D == 3 ? s * s * s : s * s, sf = sc / s, nc = D == 3 ? n * n * n : n * n, nf = nc / n;
	const int    lo2 = D * sc / 2, per = lo2 + D * sf; // work items per auxiliary patch: the LO pairs, then the HI values
	const size_t FVs = (size_t) D * sc + (size_t) D * sf, total = (size_t) G.Q * per;
	for (size_t idx = (size_t) blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t) gridDim.x * blockDim.x) {
		const int      q = (int) (idx / per), w = (int) (idx % per);
		const int32_t *o = G.origin + (size_t) q * 3;
		double        *ap = aux + (size_t) q * FVs;
		if (w < lo2) { // LO_a: the cell split, block a
			const int a = w / (sc / 2), j = w % (sc / 2);
			reinterpret_cast<double2 *>(ap + (size_t) a * sc)[j] = reinterpret_cast<const double2 *>(big + (size_t) a * nc)[ccBigPair(G, q, j)];
			continue;
		}
		const int a = (w - lo2) / sf, t = (w - lo2) % sf;
		// the face coordinate t = (t0, t1) runs over the axes other than a, in order
		int c[3] = {0, 0, 0}, b0 = a == 0 ? 1 : 0, b1 = a == 2 ? 1 : 2;
		c[b0] = o[b0] + t % s;
		if (D == 3) c[b1] = o[b1] + t / s;
		const int top = o[a] + s; // the auxiliary patch's upper a-face as a plane of the big patch
		double    v;
		if (top < n) {
			c[a] = top;
			v    = big[(size_t) a * nc + c[0] + (size_t) n * (c[1] + (size_t) n * c[2])];
		} else {
			const int T = D == 3 ? c[b0] + n * c[b1] : c[b0];
			v           = big[(size_t) D * nc + (size_t) a * nf + T];
		}
		ap[(size_t) D * sc + (size_t) a * sf + t] = v;
	}
}
} // namespace te
