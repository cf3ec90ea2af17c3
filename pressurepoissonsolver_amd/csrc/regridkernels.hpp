// Regridding on the device: the per-patch error indicator te_patch_indicator and the transfer of a level-0
// vector from one mesh to the next, te_vec_regrid. Neither has a counterpart in the reference.
//
// Indicator. out[p] = max over the axes a and over the cells c of patch p whose index along a lies in 1 .. n-2 of
// |(u[c - e_a] + u[c + e_a]) - 2 u[c]|. Patch-local. 2 u is exact, so the value is the same with or without FMA contraction, and a
// maximum does not depend on order: bit-reproducible. One workgroup per patch or z-slab; a thread owns pairs of cells in x (16-byte
// loads of the centre and of its y and z neighbours, two scalars for the x neighbours), reduces in registers, then wave shuffles,
// then LDS, then one value per workgroup. No atomics. Algorithmic bytes per site: 8 read.
//
// Transfer. One row of RG_ROW int32 per DESTINATION patch: [0] kind, [1] orthant, [2 ..] source patches.
//   RG_COPY     u_dst = source patch [2], bit for bit                                                         (16 B per site)
//   RG_REFINE   the patch is orthant [1] of source patch [2]. Extended block E on -1 .. n per axis, filled x then y then z:
//               E[-1] = (3 e[0] - 3 e[1]) + e[2], E[n] = (3 e[n-1] - 3 e[n-2]) + e[n-3], later axes extrapolating the ghosts of earlier
//               ones (tensor product; every face one-sided, so no ghost of the source hierarchy is read). Then per axis, with
//               c = (i + o_a n) >> 1 and d = -1 (i even) / +1 (i odd): v <- (30 E[c] + 5 E[c + d] - 3 E[c - d]) / 32, x then y then z:
//               quad3 and the march of k_prolong_quadratic3d.                                          (8 + 1 B per site plus ring)
//   RG_COARSEN  source patches [2 + o] are the 2^D children: restrictCell / restrictCell2d, the bits of k_restrict3d / 2d (72 B per
//               coarse cell in 3D).
// 3D, k_regrid3d<N, ZS>: one workgroup per destination patch or z-slab of it, so every cell has one writer and the kind is uniform
// per workgroup. The refine branch stages the (N/2 + 2)^2 x (ZL/2 + 2) ring block of the octant in LDS: the in-patch entries first
// (batches of four loads, all issued before the first is stored), then, behind a barrier each, the x, y and z ghost planes from the
// entries already there; then the march with 16-byte stores. 2D, k_regrid2d: one thread per pair of cells, everything from global
// memory.
#pragma once
#include "prolongkernels.hpp"

namespace te
{
enum RegridKind : int32_t { RG_COPY = 0, RG_REFINE = 1, RG_COARSEN = 2 };
constexpr int RG_ROW = 10;

__device__ __forceinline__ double secondDiff(double lo, double c, double hi) { return fabs((lo + hi) - 2.0 * c); }

// max over the workgroup (TPB threads, a multiple of 64) of v >= 0; the result is valid in thread 0
template <int TPB> __device__ __forceinline__ double blockMax(double v, double *red)
{
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, 64));
	constexpr int NW = TPB / 64;
	if (NW == 1) return v;
	if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
	__syncthreads();
	if (threadIdx.x == 0)
#pragma unroll
		for (int w = 1; w < NW; w++) v = fmax(v, red[w]);
	return v;
}

// out[p * ZS + slab]: the indicator over the cells of the slab (their z neighbours may lie in the next slab of the same patch)
template <int N, int ZS> __global__ __launch_bounds__(256) void k_indicator3d(int P, const double *__restrict__ u, double *__restrict__ out)
{
	constexpr int NN = N * N, NNN = N * N * N, NP = NN / 2, ZL = N / ZS, HX = N / 2;
	__shared__ double red[4];
	const int work = blockIdx.x;
	if (work >= P * ZS) return;
	const int     p = work / ZS, z0 = (work % ZS) * ZL;
	const double *up = u + (size_t) p * NNN;
	double        m  = 0.0;
	for (int i = threadIdx.x; i < ZL * NP; i += 256) {
		const int     X = i % HX, y = (i / HX) % N, z = z0 + i / NP, x = 2 * X;
		const double *c = up + x + N * y + NN * z;
		const double2 v = *reinterpret_cast<const double2 *>(c);
		// x: cell x needs x >= 1 (its upper neighbour is the pair's other cell), cell x + 1 needs x + 2 <= N - 1
		if (x >= 1) m = fmax(m, secondDiff(c[-1], v.x, v.y));
		if (x + 2 <= N - 1) m = fmax(m, secondDiff(v.x, v.y, c[2]));
		if (y >= 1 && y <= N - 2) {
			const double2 a = *reinterpret_cast<const double2 *>(c - N), b = *reinterpret_cast<const double2 *>(c + N);
			m = fmax(m, fmax(secondDiff(a.x, v.x, b.x), secondDiff(a.y, v.y, b.y)));
		}
		if (z >= 1 && z <= N - 2) {
			const double2 a = *reinterpret_cast<const double2 *>(c - NN), b = *reinterpret_cast<const double2 *>(c + NN);
			m = fmax(m, fmax(secondDiff(a.x, v.x, b.x), secondDiff(a.y, v.y, b.y)));
		}
	}
	m = blockMax<256>(m, red);
	if (threadIdx.x == 0) out[work] = m;
}

// the slabs' values of a patch, in slab order
static __global__ __launch_bounds__(256) void k_indicator_final(int P, int zs, const double *__restrict__ part, double *__restrict__ out)
{
	const int p = blockIdx.x * blockDim.x + threadIdx.x;
	if (p >= P) return;
	double m = part[(size_t) p * zs];
	for (int s = 1; s < zs; s++) m = fmax(m, part[(size_t) p * zs + s]);
	out[p] = m;
}

static __global__ __launch_bounds__(256) void k_indicator2d(int n, int P, const double *__restrict__ u, double *__restrict__ out)
{
	__shared__ double red[4];
	const int p = blockIdx.x;
	if (p >= P) return;
	const int     h = n / 2;
	const double *up = u + (size_t) p * n * n;
	double        m  = 0.0;
	for (int i = threadIdx.x; i < n * h; i += 256) {
		const int     x = 2 * (i % h), y = i / h;
		const double *c = up + x + n * y;
		const double2 v = *reinterpret_cast<const double2 *>(c);
		if (x >= 1) m = fmax(m, secondDiff(c[-1], v.x, v.y));
		if (x + 2 <= n - 1) m = fmax(m, secondDiff(v.x, v.y, c[2]));
		if (y >= 1 && y <= n - 2) {
			const double2 a = *reinterpret_cast<const double2 *>(c - n), b = *reinterpret_cast<const double2 *>(c + n);
			m = fmax(m, fmax(secondDiff(a.x, v.x, b.x), secondDiff(a.y, v.y, b.y)));
		}
	}
	m = blockMax<256>(m, red);
	if (threadIdx.x == 0) out[p] = m;
}

__device__ __forceinline__ double extrap3(double m, double m1, double m2) { return (3.0 * m - 3.0 * m1) + m2; }

template <int N, int ZS>
__global__ __launch_bounds__(Tile3<N>::TPB) void k_regrid3d(int Pd, const int32_t *__restrict__ map, const double *__restrict__ src,
                                                             double *__restrict__ dst)
{
	using T           = Tile3<N>;
	constexpr int TPB = T::TPB, H = T::H, NP = T::NP;
	constexpr int NN = N * N, NNN = N * N * N;
	constexpr int ZL = N / ZS;   // destination planes of a slab
	constexpr int CZ = ZL / 2;   // source planes under them (refine)
	constexpr int W = H + 2, WW = W * W, TOT = (CZ + 2) * WW;
	static_assert(ZL % 2 == 0 && ZL >= 4 && N >= 4, "whole coarse planes, and three cells inside every face of the ring block");
	const int nblocks = Pd * ZS;
	const int work    = xcdRemap(blockIdx.x, nblocks);
	if (work >= nblocks) return;
	const int      pd = work / ZS, z0 = (work % ZS) * ZL, tid = threadIdx.x;
	const int32_t *row = map + (size_t) pd * RG_ROW;
	const int      kind = row[0], o = row[1];
	double2       *up2 = reinterpret_cast<double2 *>(dst + (size_t) pd * NNN) + z0 * NP;

	if (kind == RG_COPY) {
		const double2 *e2 = reinterpret_cast<const double2 *>(src + (size_t) row[2] * NNN) + z0 * NP;
		for (int base = tid; base < ZL * NP; base += 4 * TPB) {
			double2 b[4];
#pragma unroll
			for (int j = 0; j < 4; j++) b[j] = e2[base + j * TPB < ZL * NP ? base + j * TPB : 0];
#pragma unroll
			for (int j = 0; j < 4; j++)
				if (base + j * TPB < ZL * NP) up2[base + j * TPB] = b[j];
		}
		return;
	}
	if (kind == RG_COARSEN) { // a pair of coarse cells per thread and step: both lie in one child (N / 2 is even)
		for (int i = tid; i < ZL * NP; i += TPB) {
			const int x = 2 * (i % H), y = (i / H) % N, z = z0 + i / NP;
			const int ox = x >= H, oy = y >= H, oz = z >= H;
			const int hx = x - ox * H, hy = y - oy * H, hz = z - oz * H;
			const double *fp = src + (size_t) row[2 + ox + 2 * oy + 4 * oz] * NNN;
			up2[i] = double2{restrictCell<N>(fp, hx, hy, hz), restrictCell<N>(fp, hx + 1, hy, hz)};
		}
		return;
	}

	// ---- RG_REFINE: ring entry (lx, ly, lz) is cell (bx + lx, by + ly, bz + lz) of the source patch
	__shared__ double E[TOT];
	const double *ep = src + (size_t) row[2] * NNN;
	const bool    act = (T::NT == TPB) || tid < T::NT;
	const int     X = act ? tid % H : 0, Y = act ? tid / H : 0;
	const int     q[2] = {(2 * Y) * H + X, (2 * Y + 1) * H + X}; // rows 2Y, 2Y + 1 of a destination plane, as pairs in x
	const int     bx = ((o & 1) ? H : 0) - 1, by = ((o & 2) ? H : 0) - 1, bz = ((o & 4) ? H : 0) + z0 / 2 - 1;
	auto          inside = [](int c) { return c >= 0 && c < N; };
	for (int base = tid; base < TOT; base += 4 * TPB) {
		double v[4];
		bool   in[4];
#pragma unroll
		for (int j = 0; j < 4; j++) {
			const int idx = base + j * TPB;
			const int c0 = bx + idx % W, c1 = by + (idx / W) % W, c2 = bz + idx / WW;
			in[j] = idx < TOT && inside(c0) && inside(c1) && inside(c2);
			v[j]  = ep[in[j] ? c0 + N * c1 + NN * c2 : 0];
		}
#pragma unroll
		for (int j = 0; j < 4; j++)
			if (in[j]) E[base + j * TPB] = v[j];
	}
	ldsBarrier();
	{ // x ghosts: one plane of the ring (the octant touches one x face of the source patch), where y and z are inside
		const int lx = (o & 1) ? W - 1 : 0, d = (o & 1) ? -1 : 1;
		for (int i = tid; i < W * (CZ + 2); i += TPB) {
			const int ly = i % W, lz = i / W;
			if (!inside(by + ly) || !inside(bz + lz)) continue;
			double *e = E + lx + W * ly + WW * lz;
			e[0]      = extrap3(e[d], e[2 * d], e[3 * d]);
		}
	}
	ldsBarrier();
	{ // y ghosts, the x ghosts included, where z is inside
		const int ly = (o & 2) ? W - 1 : 0, d = (o & 2) ? -W : W;
		for (int i = tid; i < W * (CZ + 2); i += TPB) {
			const int lx = i % W, lz = i / W;
			if (!inside(bz + lz)) continue;
			double *e = E + lx + W * ly + WW * lz;
			e[0]      = extrap3(e[d], e[2 * d], e[3 * d]);
		}
	}
	ldsBarrier();
	{ // z ghosts, if the slab touches the z face: whole planes
		const bool lo = bz < 0, hi = bz + CZ + 1 >= N;
		if (lo || hi) {
			const int lz = lo ? 0 : CZ + 1, d = lo ? WW : -WW;
			for (int i = tid; i < WW; i += TPB) {
				double *e = E + i + WW * lz;
				e[0]      = extrap3(e[d], e[2 * d], e[3 * d]);
			}
		}
	}
	ldsBarrier();

	// ---- the march of k_prolong_quadratic3d: pm, pcur, pn = ring planes lz - 1, lz, lz + 1 interpolated in x and y
	auto planeXY = [&](int lz, double2 *pl) {
		const double *r0 = E + lz * WW + Y * W + X; // row ly - 1 = Y, column lx - 1 = X
		double2       xr[3];
#pragma unroll
		for (int r = 0; r < 3; r++) {
			const double a = r0[r * W], b = r0[r * W + 1], c = r0[r * W + 2];
			xr[r] = double2{quad3(b, a, c), quad3(b, c, a)};
		}
		pl[0] = double2{quad3(xr[1].x, xr[0].x, xr[2].x), quad3(xr[1].y, xr[0].y, xr[2].y)};
		pl[1] = double2{quad3(xr[1].x, xr[2].x, xr[0].x), quad3(xr[1].y, xr[2].y, xr[0].y)};
	};
	double2 pm[2], pcur[2], pn[2];
	planeXY(0, pcur);
	planeXY(1, pn);
#pragma unroll 2
	for (int j = 0; j < CZ; j++) {
#pragma unroll
		for (int k = 0; k < 2; k++) pm[k] = pcur[k], pcur[k] = pn[k];
		planeXY(j + 2, pn);
		if (act) {
#pragma unroll
			for (int k = 0; k < 2; k++) { // rows 2Y + k of destination planes 2j (towards the plane below) and 2j + 1 (above)
				up2[(2 * j) * NP + q[k]]     = double2{quad3(pcur[k].x, pm[k].x, pn[k].x), quad3(pcur[k].y, pm[k].y, pn[k].y)};
				up2[(2 * j + 1) * NP + q[k]] = double2{quad3(pcur[k].x, pn[k].x, pm[k].x), quad3(pcur[k].y, pn[k].y, pm[k].y)};
			}
		}
	}
}

// E of the source patch e (n x n) at (cx, cy), any index in -1 .. n: x first, then y over the x ghosts as well
__device__ __forceinline__ double regridExt2d(const double *e, int n, int cx, int cy)
{
	auto ex = [&](int y) { // E(cx, y) for y inside
		const double *r = e + (size_t) n * y;
		if (cx < 0) return extrap3(r[0], r[1], r[2]);
		if (cx >= n) return extrap3(r[n - 1], r[n - 2], r[n - 3]);
		return r[cx];
	};
	if (cy < 0) return extrap3(ex(0), ex(1), ex(2));
	if (cy >= n) return extrap3(ex(n - 1), ex(n - 2), ex(n - 3));
	return ex(cy);
}

static __global__ __launch_bounds__(256) void k_regrid2d(int n, int Pd, const int32_t *__restrict__ map, const double *__restrict__ src,
                                                         double *__restrict__ dst)
{
	const int    h = n / 2, nn = n * n;
	const size_t total = (size_t) Pd * n * h;
	for (size_t idx = (size_t) blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t) gridDim.x * blockDim.x) {
		const int      pd = (int) (idx / ((size_t) n * h)), q = (int) (idx % ((size_t) n * h));
		const int      y = q / h, X = q % h;
		const int32_t *row = map + (size_t) pd * RG_ROW;
		const int      kind = row[0], o = row[1];
		double2       *fp = reinterpret_cast<double2 *>(dst + (size_t) pd * nn + 2 * X + n * y);
		if (kind == RG_COPY) {
			*fp = *reinterpret_cast<const double2 *>(src + (size_t) row[2] * nn + 2 * X + n * y);
			continue;
		}
		if (kind == RG_COARSEN) {
			auto cell = [&](int x) { // (n / 2 may be odd: the two cells of a pair need not lie in one child)
				const int ox = x >= h, oy = y >= h;
				return restrictCell2d(src + (size_t) row[2 + ox + 2 * oy] * nn, n, x - ox * h, y - oy * h);
			};
			*fp = double2{cell(2 * X), cell(2 * X + 1)};
			continue;
		}
		const double *e = src + (size_t) row[2] * nn;
		const int     cx = X + ((o & 1) ? h : 0), cy = (y + ((o & 2) ? n : 0)) >> 1, dy = (y & 1) ? 1 : -1;
		double2       xr[3]; // rows cy, cy + dy, cy - dy
#pragma unroll
		for (int r = 0; r < 3; r++) {
			const int    yy = r == 0 ? cy : (r == 1 ? cy + dy : cy - dy);
			const double a = regridExt2d(e, n, cx - 1, yy), b = regridExt2d(e, n, cx, yy), c = regridExt2d(e, n, cx + 1, yy);
			xr[r] = double2{quad3(b, a, c), quad3(b, c, a)};
		}
		*fp = double2{quad3(xr[0].x, xr[1].x, xr[2].x), quad3(xr[0].y, xr[1].y, xr[2].y)};
	}
}
} // namespace te
