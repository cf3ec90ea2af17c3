// Boundary data on the device: the values a driver prescribes on the physical faces of the domain live in a BOUNDARY VECTOR -- one
// block of n^(dim-1) doubles per physical face of this rank's patches, faces numbered in (patch, side) order (mesh.hpp bfaceIndex),
// a block laid out like an interface block of the Schur route: the face's remaining axes in order, the first fastest (side on x:
// [z][y]; on y: [z][x]; on z: [y][x]; 2D: one row). k_boundary_rhs folds such a vector into a right-hand side the way
// Init::initDirichlet / Init::initNeumann fold their callbacks (apps/shared/Init.cpp:186-240, :89-146):
//   Dirichlet face  f -= 2 g / h^2          Neumann face  f += g_n / h (lower side),  f -= g_n / h (upper side)
// with g_n the derivative ALONG THE AXIS (not the outward normal) and h the patch's spacing on that axis; k_boundary_sample fills
// one with the canned problems' data (Prob3 / Prob2 of initkernels.hpp). Replaces the host loops over getLocalData
// (thunderegg/HipInit.h) for data that changes every time step; nothing in the reference runs on a device.
//
// Bytes: the fold reads and writes the face layers of patches that touch the boundary and reads the boundary vector once --
// 16 B per touched site + 8 B per boundary value, on 2 dim / n of a boundary patch's sites and none of an interior patch's
// (one 4-byte table row per (patch, side) decides). At 512^3 in 32^3 patches: 6 * 512^2 face cells of 1.3e8 sites, 38 MB of traffic
// against the 2.1 GB of one pass over f.
#pragma once
#include "initkernels.hpp"
#include "table_layout.hpp"

namespace te
{
struct BcGeom {
	int            n, P;
	const double  *starts;    // [P][3]
	const double  *h;         // [P][3]
	const int32_t *face_kind; // [P][2 dim]
	const int32_t *bface;     // [P][2 dim] block of the face in a boundary vector, -1 on a face with a neighbour
};

// cell j of the layer along side s of an n^D patch: ci[] = its cell index, the fixed axis at 0 or n - 1
template <int D> __device__ __forceinline__ void bcFaceCell(int n, int s, int j, int *ci)
{
	const int ax = s >> 1;
#pragma unroll
	for (int a = 0; a < D; a++) {
		if (a == ax) {
			ci[a] = (s & 1) ? n - 1 : 0;
		} else {
			ci[a] = j % n;
			j /= n;
		}
	}
}
// where cell ci[] sits in the block of side s (the inverse of bcFaceCell)
template <int D> __device__ __forceinline__ int bcBlockPos(int n, int s, const int *ci)
{
	const int ax = s >> 1;
	int       j = 0, m = 1;
#pragma unroll
	for (int a = 0; a < D; a++)
		if (a != ax) {
			j += m * ci[a];
			m *= n;
		}
	return j;
}

// One workgroup per (patch, side), its threads over the cells of that face layer. A cell of an edge or a corner lies in up to D
// layers and receives up to D terms: its OWNER is the thread of the lowest side whose layer holds it -- whatever that side's
// kind --, and the owner alone applies the terms of all the cell's physical sides in side order (the order of k_init3d). No two
// threads write one cell, no atomics, the same bits every run.
template <int D> __global__ __launch_bounds__(256) void k_boundary_rhs(BcGeom G, const double *__restrict__ bdata, double *__restrict__ f)
{
	constexpr int NS = 2 * D;
	const int     n = G.n, p = blockIdx.x / NS, s = blockIdx.x % NS;
	if (p >= G.P) return;
	int  bf[NS], kind[NS];
	bool any = false;
#pragma unroll
	for (int t = 0; t < NS; t++) {
		bf[t]   = G.bface[(size_t) p * NS + t];
		kind[t] = G.face_kind[(size_t) p * NS + t];
		any |= bf[t] >= 0;
	}
	if (!any) return; // (an interior patch)
	int nf = 1, nc = 1;
#pragma unroll
	for (int a = 0; a < D; a++) {
		nc *= n;
		if (a) nf *= n;
	}
	const double *h = G.h + (size_t) p * 3;
	for (int j = threadIdx.x; j < nf; j += 256) {
		int ci[D];
		bcFaceCell<D>(n, s, j, ci);
		bool owner = true, touched = false;
#pragma unroll
		for (int t = 0; t < NS; t++) {
			const bool on = ci[t >> 1] == ((t & 1) ? n - 1 : 0);
			if (t < s && on) owner = false;
			touched |= on && bf[t] >= 0;
		}
		if (!owner || !touched) continue;
		size_t c = 0, m = 1;
#pragma unroll
		for (int a = 0; a < D; a++) {
			c += m * ci[a];
			m *= n;
		}
		const size_t at = (size_t) p * nc + c;
		double       v  = f[at];
#pragma unroll
		for (int t = 0; t < NS; t++) {
			const int ax = t >> 1, hi = t & 1;
			if (ci[ax] != (hi ? n - 1 : 0) || bf[t] < 0) continue;
			const double b = bdata[(size_t) bf[t] * nf + bcBlockPos<D>(n, t, ci)];
			if (kind[t] == FACE_NEUMANN) {
				const double g = b / h[ax];
				v              = hi ? v - g : v + g;
			} else {
				v -= 2 * b / (h[ax] * h[ax]);
			}
		}
		f[at] = v;
	}
}

// te_boundary_restrict: the boundary vector of the next coarser level. Each entry of a coarse block is the mean of the 2^(D-1)
// fine entries that cover it -- 3D ((a + b) + (c + d)) * 0.25 with a, b adjacent along the face's lower remaining axis, 2D
// (a + b) * 0.5 --, taken from the block of the child in that quadrant (tab: level_tables.hpp brestrict); a patch that copies
// through hands its block on bit for bit. One workgroup per COARSE block, one thread per entry: one writer, no atomics. Dirichlet
// values and Neumann derivatives restrict alike. 8 B written + 8 * 2^(D-1) B read per coarse value.
template <int D>
__global__ __launch_bounds__(256) void k_boundary_restrict(int n, int ncb, const int32_t *__restrict__ tab, const double *__restrict__ fine,
                                                            double *__restrict__ coarse)
{
	const int cb = blockIdx.x;
	if (cb >= ncb) return;
	const int32_t *row = tab + (size_t) cb * 5;
	const int      h = n / 2, nf = D == 3 ? n * n : n;
	double        *dst = coarse + (size_t) cb * nf;
	if (row[0]) {
		const double *src = fine + (size_t) row[1] * nf;
		for (int j = threadIdx.x; j < nf; j += 256) dst[j] = src[j];
		return;
	}
	for (int j = threadIdx.x; j < nf; j += 256) {
		const int j0 = j % n, j1 = j / n; // (2D: j1 = 0)
		const int u0 = j0 >= h, u1 = D == 3 && j1 >= h;
		const double *src = fine + (size_t) row[1 + u0 + 2 * u1] * nf + 2 * (j0 - u0 * h);
		if (D == 3) {
			src += (size_t) n * 2 * (j1 - u1 * h);
			dst[j] = ((src[0] + src[1]) + (src[n] + src[n + 1])) * 0.25;
		} else {
			dst[j] = (src[0] + src[1]) * 0.5;
		}
	}
}

// the canned problems' boundary data: the exact solution at the face point on a Dirichlet face, its derivative along the face's
// axis on a Neumann face (what k_init3d / k_init2d fold in). One workgroup per (patch, side).
template <int D, int PROB> __global__ __launch_bounds__(256) void k_boundary_sample(BcGeom G, double *__restrict__ bdata)
{
	constexpr int NS = 2 * D;
	const int     n = G.n, p = blockIdx.x / NS, s = blockIdx.x % NS;
	if (p >= G.P) return;
	const int bf = G.bface[(size_t) p * NS + s];
	if (bf < 0) return;
	const bool neumann = G.face_kind[(size_t) p * NS + s] == FACE_NEUMANN;
	int        nf      = 1;
#pragma unroll
	for (int a = 1; a < D; a++) nf *= n;
	const double *st = G.starts + (size_t) p * 3, *h = G.h + (size_t) p * 3;
	const int     ax = s >> 1;
	for (int j = threadIdx.x; j < nf; j += 256) {
		int ci[D];
		bcFaceCell<D>(n, s, j, ci);
		ci[ax] = (s & 1) ? n : -1; // (the face itself: Init.cpp:25-50)
		double x[3] = {0, 0, 0};
#pragma unroll
		for (int a = 0; a < D; a++) x[a] = initCoord(st[a], h[a], n, ci[a]);
		double v;
		if (D == 3)
			v = neumann ? Prob3<PROB>::normal(ax, x[0], x[1], x[2]) : Prob3<PROB>::exact(x[0], x[1], x[2]);
		else
			v = neumann ? Prob2<PROB>::normal(ax, x[0], x[1]) : Prob2<PROB>::exact(x[0], x[1]);
		bdata[(size_t) bf * nf + j] = v;
	}
}
} // namespace te
