// Kernels of the Schur-complement route (gmg_schur.hip): the interface vector gamma -- one block of n^(D-1) values per
// interface, SchurHelper.h:377-397 order -- to the patches' interface terms and back.
//   k_iface_corr   gamma -> corr[P][2D][n^(D-1)] = 2 gamma / h^2 on every face with a neighbour, 0 on physical faces: what
//                  k_face_corr3d makes of an iterate u when gamma = Interp(u), so every patch-solve kernel takes it unchanged
//   k_iface_rhs    out = f -+ corr on the face layers, sides in the reference's order W,E,S,N,B,T (StarPatchOp.h:185-203)
//   k_iface_interp u (or the six face layers of a patch solve, [P][6][n^2]) -> gamma: SchurHelper::interpolateToInterface
//                  (SchurHelper.h:333-343, TriLinInterp.cpp:60-172, BilinearInterpolator.cpp:61-117) in gather form: one
//                  workgroup per interface block sums its contributions in (patch, side) order -- no atomics, the order of
//                  the reference's own scatter loop, deterministic
// Face coordinates (a, b): the two remaining axes in ascending order, cell a + n b of the block (Vector.h:152-177).
#pragma once
#include "mesh.hpp"
#include <hip/hip_runtime.h>

namespace te
{
// offset of face cell (a, b) of side s inside a patch, on the face layer itself
template <int DIM> __device__ __forceinline__ int ifaceCell(int n, int s, int a, int b)
{
	const int ax = s >> 1, pos = (s & 1) ? n - 1 : 0;
	if (DIM == 2) return ax == 0 ? pos + a * n : pos * n + a;
	if (ax == 0) return pos + a * n + b * n * n;
	if (ax == 1) return pos * n + a + b * n * n;
	return pos * n * n + a + b * n;
}

template <int DIM>
__global__ __launch_bounds__(256) void k_iface_corr(int n, const int32_t *__restrict__ own, const double *__restrict__ rh2,
                                                    const double *__restrict__ gamma, double *__restrict__ corr)
{
	constexpr int NS = 2 * DIM;
	const int     nf = DIM == 3 ? n * n : n;
	const int     p = blockIdx.x / NS, s = blockIdx.x % NS;
	const int     i = own[blockIdx.x];
	const double  rh = rh2[(size_t) p * 3 + (s >> 1)];
	double       *c  = corr + (size_t) blockIdx.x * nf;
	for (int k = threadIdx.x; k < nf; k += blockDim.x) c[k] = i >= 0 ? 2.0 * rh * gamma[(size_t) i * nf + k] : 0.0;
}

// out = f - corr (ADD: f + corr) on the face layers, f elsewhere; f == null: a zero right-hand side. One thread per cell.
template <int DIM, bool ADD>
__global__ __launch_bounds__(256) void k_iface_rhs(size_t total, int n, const double *__restrict__ f, const double *__restrict__ corr,
                                                   double *out)
{
	const int nf = DIM == 3 ? n * n : n, nc = nf * n;
	for (size_t c = (size_t) blockIdx.x * blockDim.x + threadIdx.x; c < total; c += (size_t) gridDim.x * blockDim.x) {
		const size_t  p = c / nc;
		const int     r = (int) (c - p * nc), x = r % n, y = (r / n) % n, z = DIM == 3 ? r / (n * n) : 0;
		const double *cp = corr + p * 2 * DIM * nf;
		double        v  = f ? f[c] : 0.0;
		auto          term = [&](int s, int k) { v = ADD ? v + cp[s * nf + k] : v - cp[s * nf + k]; };
		if (x == 0) term(0, DIM == 3 ? y + n * z : y);
		if (x == n - 1) term(1, DIM == 3 ? y + n * z : y);
		if (y == 0) term(2, DIM == 3 ? x + n * z : x);
		if (y == n - 1) term(3, DIM == 3 ? x + n * z : x);
		if (DIM == 3 && z == 0) term(4, x + n * y);
		if (DIM == 3 && z == n - 1) term(5, x + n * y);
		out[c] = v;
	}
}

// contrib[k] = (patch, side, IfaceKind, quadrant) for k in [start[i], start[i+1]). F6: src is [P][6][n^2] face layers.
template <int DIM, bool F6>
__global__ __launch_bounds__(256) void k_iface_interp(int n, const int32_t *__restrict__ start, const int4 *__restrict__ contrib,
                                                      const double *__restrict__ src, double *__restrict__ gamma)
{
	const int    nf = DIM == 3 ? n * n : n;
	const size_t nc = (size_t) nf * n;
	const int    i = blockIdx.x, k0 = start[i], k1 = start[i + 1];
	for (int e = threadIdx.x; e < nf; e += blockDim.x) {
		const int a = DIM == 3 ? e % n : e, b = DIM == 3 ? e / n : 0;
		double    acc = 0.0;
		for (int k = k0; k < k1; k++) {
			const int4 c = contrib[k];
			const int  p = c.x, s = c.y, kind = c.z, q = c.w;
			auto       sl = [&](int fa, int fb) {
                return F6 ? src[((size_t) p * 6 + s) * nf + fa + n * fb] : src[(size_t) p * nc + ifaceCell<DIM>(n, s, fa, fb)];
			};
			if (DIM == 3) {
				if (kind == IF_NORMAL) {
					acc += 0.5 * sl(a, b); // TriLinInterp.cpp:78-84
				} else if (kind == IF_FINE_TO_FINE) { // :85-98
					const int    a0 = a & ~1, b0 = b & ~1, w = (a & 1) + 2 * (b & 1);
					const double va = sl(a0, b0), vb = sl(a0 + 1, b0), vc = sl(a0, b0 + 1), vd = sl(a0 + 1, b0 + 1);
					if (w == 0) acc += (11 * va - vb - vc - vd) / 12.0;
					else if (w == 1) acc += (-va + 11 * vb - vc - vd) / 12.0;
					else if (w == 2) acc += (-va - vb + 11 * vc - vd) / 12.0;
					else acc += (-va - vb - vc + 11 * vd) / 12.0;
				} else if (kind == IF_FINE_TO_COARSE) { // :138-170, the four fine cells of this coarse cell in their loop order
					const int fa = 2 * a - ((q & 1) ? n : 0), fb = 2 * b - ((q & 2) ? n : 0);
					if (fa >= 0 && fa < n && fb >= 0 && fb < n) {
						acc += 1.0 / 6.0 * sl(fa, fb);
						acc += 1.0 / 6.0 * sl(fa + 1, fb);
						acc += 1.0 / 6.0 * sl(fa, fb + 1);
						acc += 1.0 / 6.0 * sl(fa + 1, fb + 1);
					}
				} else if (kind == IF_COARSE_TO_COARSE) {
					acc += 2.0 / 6.0 * sl(a, b); // :131-137
				} else { // IF_COARSE_TO_FINE :99-130
					acc += 4.0 * sl((a + ((q & 1) ? n : 0)) / 2, (b + ((q & 2) ? n : 0)) / 2) / 12.0;
				}
			} else {
				if (kind == IF_NORMAL) {
					acc += 0.5 * sl(a, 0); // BilinearInterpolator.cpp:71-75
				} else if (kind == IF_FINE_TO_FINE) { // :95-103
					acc += 5.0 / 6 * sl(a, 0) - 1.0 / 6 * sl(a ^ 1, 0);
				} else if (kind == IF_FINE_TO_COARSE) { // :82-94
					const int fa = 2 * a - ((q & 1) ? n : 0);
					if (fa >= 0 && fa < n) acc += 1.0 / 3 * sl(fa, 0) + 1.0 / 3 * sl(fa + 1, 0);
				} else if (kind == IF_COARSE_TO_COARSE) {
					acc += 1.0 / 3 * sl(a, 0); // :76-81
				} else { // :104-115
					acc += 2.0 / 6 * sl(((q ? n : 0) + a) / 2, 0);
				}
			}
		}
		gamma[(size_t) i * nf + e] = acc;
	}
}
} // namespace te
