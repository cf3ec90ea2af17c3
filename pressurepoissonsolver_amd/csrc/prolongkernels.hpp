// Linear (trilinear / bilinear) prolongation, the second interpolator of a cycle next to DrctIntp (k_prolong3d / k_prolong2d). It
// stands behind the reference's GMG/TriLinIntp.h (which its build leaves out), restated patch-locally:
//
//   extended block E of a coarse patch, indices -1 .. n per axis
//     all indices in range       E = e
//     one axis out of range      the ghost the operator's stencil reads there for e (homogeneous data): the neighbour's cell, the ghost
//                                slot of a coarse/fine or remote face (2 gamma - m), -m on a Dirichlet face, +m on a Neumann face
//     k >= 2 axes out of range   m = the patch's own cell with the indices clamped: the sum over the out-of-range axes, in ascending
//                                order, of the face ghost of m through that axis, minus (k - 1) m. No edge or corner neighbour is read.
//   fine cell i of a child in orthant o, per axis a: c = (i + o_a n) >> 1, d = -1 (i even) / +1 (i odd),
//     v <- 0.75 E[c] + 0.25 E[c + d], x then y then z; u += v.        A patch that copies through (orthant -1): u += e.
//
// 3D, k_prolong_linear3d<N, ZS>: fine-patch driven -- one workgroup per fine patch or z-slab of it (exactly one writer per fine cell,
// no atomics). The ring block of the parent's octant that the slab needs, (N/2 + 2)^2 x (ZL/2 + 2) values, is staged in LDS: first
// the entries with at most one axis out of range (loads in batches of four, all in flight before the first is stored), then, behind
// a barrier, the edge and corner entries from the face entries already there. A thread then owns one coarse column: it interpolates
// a coarse plane in x and y from nine LDS values, keeps three such planes in registers and forms two fine planes per step. The fine
// read-modify-write moves double2 (16 B); the fine planes of a step are requested two steps ahead into a two-slot register ring, so
// no load is consumed by the step that requested it. Algorithmic bytes per fine site: 16 (u) + 1 (e) + halos.
// 2D, k_prolong_linear2d: the simple form of k_stencil2d, one thread per pair of fine cells, coarse values and ghosts from global memory.
#pragma once
#include "march3d.hpp"
#include "kernels2d.hpp"

namespace te
{
template <int N, int ZS>
__global__ __launch_bounds__(Tile3<N>::TPB) void k_prolong_linear3d(int Pf, LevelDev C, const int32_t *__restrict__ parent,
                                                                     const int32_t *__restrict__ orth, const double *__restrict__ e, double *u)
{
	using T           = Tile3<N>;
	constexpr int TPB = T::TPB, H = T::H, NP = T::NP;
	constexpr int NN = N * N, NNN = N * N * N;
	constexpr int ZL = N / ZS;   // fine planes of a slab
	constexpr int CZ = ZL / 2;   // coarse planes under them
	constexpr int W = H + 2, WW = W * W, TOT = (CZ + 2) * WW;
	static_assert(ZL % 4 == 0 && ZL >= 4, "two coarse planes per iteration of the march");
	const int nblocks = Pf * ZS;
	const int work    = xcdRemap(blockIdx.x, nblocks);
	if (work >= nblocks) return;
	const int pf = work / ZS, z0 = (work % ZS) * ZL, tid = threadIdx.x;
	const int o = orth[pf], pc = parent[pf];
	double2  *up2 = reinterpret_cast<double2 *>(u + (size_t) pf * NNN) + z0 * NP;
	const double *ep = e + (size_t) pc * NNN;

	if (o < 0) { // copy-through: u += e, cell by cell
		const double2 *e2 = reinterpret_cast<const double2 *>(ep) + z0 * NP;
		for (int base = tid; base < ZL * NP; base += 4 * TPB) {
			double2 a[4], b[4];
#pragma unroll
			for (int j = 0; j < 4; j++) {
				const int i = base + j * TPB < ZL * NP ? base + j * TPB : 0;
				a[j] = up2[i];
				b[j] = e2[i];
			}
#pragma unroll
			for (int j = 0; j < 4; j++)
				if (base + j * TPB < ZL * NP) up2[base + j * TPB] = double2{a[j].x + b[j].x, a[j].y + b[j].y};
		}
		return;
	}

	__shared__ double E[TOT];

	const bool act = (T::NT == TPB) || tid < T::NT;
	const int  X = act ? tid % H : 0, Y = act ? tid / H : 0;
	// this thread's four pairs of a step: fine planes 2j, 2j + 1 of the slab, rows 2Y, 2Y + 1
	const int q[2] = {(2 * Y) * H + X, (2 * Y + 1) * H + X};
	double2   ur[2][4];
#pragma unroll
	for (int i = 0; i < 2; i++) {
#pragma unroll
		for (int k = 0; k < 4; k++) ur[i][k] = up2[(2 * i + (k >> 1)) * NP + q[k & 1]];
		__builtin_amdgcn_sched_barrier(0);
	}

	// ---- the ring block: entry (lx, ly, lz) is coarse cell (bx + lx, by + ly, bz + lz) of the parent
	const Reg6 fk(C.face_kind + (size_t) pc * 6), fs(C.face_src + (size_t) pc * 6);
	const int  bx = ((o & 1) ? H : 0) - 1, by = ((o & 2) ? H : 0) - 1, bz = ((o & 4) ? H : 0) + z0 / 2 - 1;
	auto       clampN = [](int c) { return c < 0 ? 0 : (c >= N ? N - 1 : c); };
	for (int base = tid; base < TOT; base += 4 * TPB) {
		double v[4], s[4];
#pragma unroll
		for (int j = 0; j < 4; j++) {
			const int  idx = base + j * TPB;
			const int  lx = idx % W, ly = (idx / W) % W, lz = idx / WW;
			const int  c[3]   = {bx + lx, by + ly, bz + lz};
			const int  cl[3]  = {clampN(c[0]), clampN(c[1]), clampN(c[2])};
			const bool out[3] = {c[0] != cl[0], c[1] != cl[1], c[2] != cl[2]};
			const int  k      = (int) out[0] + (int) out[1] + (int) out[2];
			const double *p = ep + cl[0] + N * cl[1] + NN * cl[2]; // the cell itself, or m just inside the face
			s[j]            = 1.0;
			if (k == 1 && idx < TOT) {
				const int a    = out[0] ? 0 : (out[1] ? 1 : 2);
				const int upr  = c[a] >= N;
				const int side = 2 * a + upr;
				const int kind = fk[side], src = fs[side];
				const int fa = a == 0 ? cl[1] : cl[0], fb = a == 2 ? cl[1] : cl[2]; // the face's two other axes, in order
				if (kind == FACE_LOCAL) {
					int nb[3] = {cl[0], cl[1], cl[2]};
					nb[a]     = upr ? 0 : N - 1;
					p         = e + (size_t) src * NNN + nb[0] + N * nb[1] + NN * nb[2];
				}
				if (kind == FACE_GHOST) p = C.ghost + (size_t) src * NN + fa + N * fb;
				if (kind == FACE_DIRICHLET) s[j] = -1.0;
			}
			v[j] = *p;
		}
#pragma unroll
		for (int j = 0; j < 4; j++)
			if (base + j * TPB < TOT) E[base + j * TPB] = s[j] * v[j];
	}
	ldsBarrier();
	// edges and corners of the parent that the ring touches: from the face entries (one axis out of range, the others clamped)
	for (int idx = tid; idx < TOT; idx += TPB) {
		const int  lx = idx % W, ly = (idx / W) % W, lz = idx / WW;
		const int  l[3]   = {lx, ly, lz};
		const int  c[3]   = {bx + lx, by + ly, bz + lz};
		const bool out[3] = {c[0] < 0 || c[0] >= N, c[1] < 0 || c[1] >= N, c[2] < 0 || c[2] >= N};
		if ((int) out[0] + (int) out[1] + (int) out[2] < 2) continue;
		int li[3]; // the clamped cell's entry
#pragma unroll
		for (int a = 0; a < 3; a++) li[a] = out[a] ? (c[a] < 0 ? l[a] + 1 : l[a] - 1) : l[a];
		const double m   = E[li[0] + W * li[1] + WW * li[2]];
		double       tot = -2.0 * m;
		tot += out[0] ? E[l[0] + W * li[1] + WW * li[2]] : m;
		tot += out[1] ? E[li[0] + W * l[1] + WW * li[2]] : m;
		tot += out[2] ? E[li[0] + W * li[1] + WW * l[2]] : m;
		E[idx] = tot;
	}
	ldsBarrier();

	// ---- the march: pm, pc_, pn = coarse planes lz - 1, lz, lz + 1 interpolated in x and y: [fine row 2Y | 2Y + 1] as pairs in x
	auto planeXY = [&](int lz, double2 *pl) {
		const double *r0 = E + lz * WW + Y * W + X; // row ly - 1 = Y, column lx - 1 = X
		double2       xr[3];
#pragma unroll
		for (int r = 0; r < 3; r++) {
			const double a = r0[r * W], b = r0[r * W + 1], c = r0[r * W + 2];
			xr[r] = double2{0.75 * b + 0.25 * a, 0.75 * b + 0.25 * c};
		}
		pl[0] = double2{0.75 * xr[1].x + 0.25 * xr[0].x, 0.75 * xr[1].y + 0.25 * xr[0].y};
		pl[1] = double2{0.75 * xr[1].x + 0.25 * xr[2].x, 0.75 * xr[1].y + 0.25 * xr[2].y};
	};
	double2 pm[2], pcur[2], pn[2];
	planeXY(0, pcur);
	planeXY(1, pn);
	auto step = [&](auto par, auto refill, int j) {
		constexpr int  PAR    = decltype(par)::value; // j & 1
		constexpr bool REFILL = decltype(refill)::value;
		double2        uc[4];
#pragma unroll
		for (int k = 0; k < 4; k++) {
			uc[k] = takeRegs(ur[PAR][k]);
			if (REFILL) ur[PAR][k] = up2[(2 * (j + 2) + (k >> 1)) * NP + q[k & 1]];
		}
#pragma unroll
		for (int k = 0; k < 2; k++) pm[k] = pcur[k], pcur[k] = pn[k];
		planeXY(j + 2, pn);
		if (act) {
#pragma unroll
			for (int k = 0; k < 2; k++) { // rows 2Y + k of fine planes 2j (towards the plane below) and 2j + 1 (above)
				const double2 lo{0.75 * pcur[k].x + 0.25 * pm[k].x, 0.75 * pcur[k].y + 0.25 * pm[k].y};
				const double2 hi{0.75 * pcur[k].x + 0.25 * pn[k].x, 0.75 * pcur[k].y + 0.25 * pn[k].y};
				up2[(2 * j) * NP + q[k]]     = double2{uc[k].x + lo.x, uc[k].y + lo.y};
				up2[(2 * j + 1) * NP + q[k]] = double2{uc[2 + k].x + hi.x, uc[2 + k].y + hi.y};
			}
		}
	};
	using B0 = std::integral_constant<int, 0>;
	using B1 = std::integral_constant<int, 1>;
#pragma unroll 1
	for (int j = 0; j < CZ - 2; j += 2) {
		step(B0{}, std::true_type{}, j);
		step(B1{}, std::true_type{}, j + 1);
	}
	step(B0{}, std::false_type{}, CZ - 2);
	step(B1{}, std::false_type{}, CZ - 1);
}

// E of coarse patch pc at (cx, cy), any index in -1 .. n (2D: the rule above with two axes)
__device__ __forceinline__ double extended2d(const Level2D &C, const double *e, int pc, int cx, int cy)
{
	const int    n = C.n;
	const bool   ox = cx < 0 || cx >= n, oy = cy < 0 || cy >= n;
	const int    clx = cx < 0 ? 0 : (cx >= n ? n - 1 : cx), cly = cy < 0 ? 0 : (cy >= n ? n - 1 : cy);
	const double m = e[(size_t) pc * n * n + clx + n * cly];
	if (!ox && !oy) return m;
	const double gx = ox ? ghost2d(C, e, pc, cx < 0 ? 0 : 1, cly, m, false) : m;
	const double gy = oy ? ghost2d(C, e, pc, cy < 0 ? 2 : 3, clx, m, false) : m;
	if (ox && oy) return (-m + gx) + gy;
	return ox ? gx : gy;
}
static __global__ __launch_bounds__(256) void k_prolong_linear2d(Level2D C, int Pf, const int32_t *__restrict__ parent,
                                                                 const int32_t *__restrict__ orth, const double *__restrict__ e, double *u)
{
	const int    n = C.n, h = n / 2;
	const size_t total = (size_t) Pf * n * h;
	for (size_t idx = (size_t) blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t) gridDim.x * blockDim.x) {
		const int pf = (int) (idx / ((size_t) n * h)), q = (int) (idx % ((size_t) n * h));
		const int y = q / h, X = q % h;
		const int o = orth[pf], pc = parent[pf];
		double2  *fp = reinterpret_cast<double2 *>(u + (size_t) pf * n * n + 2 * X + n * y);
		double2   v  = *fp;
		if (o < 0) {
			const double2 c = *reinterpret_cast<const double2 *>(e + (size_t) pc * n * n + 2 * X + n * y);
			v.x += c.x;
			v.y += c.y;
		} else {
			const int cx = X + ((o & 1) ? h : 0), cy = (y + ((o & 2) ? n : 0)) >> 1, dy = (y & 1) ? 1 : -1;
			double2   xr[2];
#pragma unroll
			for (int r = 0; r < 2; r++) {
				const int    yy = r ? cy + dy : cy;
				const double a = extended2d(C, e, pc, cx - 1, yy), b = extended2d(C, e, pc, cx, yy), c = extended2d(C, e, pc, cx + 1, yy);
				xr[r] = double2{0.75 * b + 0.25 * a, 0.75 * b + 0.25 * c};
			}
			v.x += 0.75 * xr[0].x + 0.25 * xr[1].x;
			v.y += 0.75 * xr[0].y + 0.25 * xr[1].y;
		}
		*fp = v;
	}
}

// ---- Quadratic FMG interpolation (te_prolong_quadratic): fine = Pi coarse. It SETS, and it interpolates a
// solution that carries boundary data, so it reads none:
//   extended block E as above with one change: on a PHYSICAL face, Dirichlet or Neumann alike, the ghost is the quadratic
//     extrapolation 3 m - 3 m1 + m2 of the first, second and third cells inside along that axis (n >= 4: they exist)
//   v <- (30 E[c] + 5 E[c + d] - 3 E[c - d]) / 32 per axis, x then y then z.       A patch that copies through: fine = coarse.
// With the extrapolated ghost the centred formula is the one-sided quadratic through the three innermost cells: quadratics are
// reproduced up to the boundary.
// 3D, k_prolong_quadratic3d<N, ZS>: the workgroups, the ring block and the march of k_prolong_linear3d. The staging pass issues
// three loads per entry from pointers chosen before them (all three the entry's own cell, weights 1, 0, 0, unless the entry is
// the ghost of a physical face: m, m1, m2 with 3, -3, 1), twelve in flight per batch of four entries. The march reads the same
// nine LDS values per plane with the other weights and keeps the same three planes. It never reads `fine`: no register ring, the
// stores stay 16-byte pairs. Algorithmic bytes per fine site: 8 written + 1 read + halos.
__device__ __forceinline__ double quad3(double c, double near, double far) { return (30.0 * c + 5.0 * near - 3.0 * far) * 0.03125; }

template <int N, int ZS>
__global__ __launch_bounds__(Tile3<N>::TPB) void k_prolong_quadratic3d(int Pf, LevelDev C, const int32_t *__restrict__ parent,
                                                                        const int32_t *__restrict__ orth, const double *__restrict__ e,
                                                                        double *__restrict__ u)
{
	using T           = Tile3<N>;
	constexpr int TPB = T::TPB, H = T::H, NP = T::NP;
	constexpr int NN = N * N, NNN = N * N * N;
	constexpr int ZL = N / ZS;   // fine planes of a slab
	constexpr int CZ = ZL / 2;   // coarse planes under them
	constexpr int W = H + 2, WW = W * W, TOT = (CZ + 2) * WW;
	static_assert(ZL % 2 == 0 && ZL >= 4 && N >= 4, "whole coarse planes, and three cells inside every face");
	const int nblocks = Pf * ZS;
	const int work    = xcdRemap(blockIdx.x, nblocks);
	if (work >= nblocks) return;
	const int pf = work / ZS, z0 = (work % ZS) * ZL, tid = threadIdx.x;
	const int o = orth[pf], pc = parent[pf];
	double2  *up2 = reinterpret_cast<double2 *>(u + (size_t) pf * NNN) + z0 * NP;
	const double *ep = e + (size_t) pc * NNN;

	if (o < 0) { // copy-through: u = e
		const double2 *e2 = reinterpret_cast<const double2 *>(ep) + z0 * NP;
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

	__shared__ double E[TOT];

	const bool act = (T::NT == TPB) || tid < T::NT;
	const int  X = act ? tid % H : 0, Y = act ? tid / H : 0;
	const int  q[2] = {(2 * Y) * H + X, (2 * Y + 1) * H + X}; // rows 2Y, 2Y + 1 of a fine plane, as pairs in x

	// ---- the ring block: entry (lx, ly, lz) is coarse cell (bx + lx, by + ly, bz + lz) of the parent
	const Reg6 fk(C.face_kind + (size_t) pc * 6), fs(C.face_src + (size_t) pc * 6);
	const int  bx = ((o & 1) ? H : 0) - 1, by = ((o & 2) ? H : 0) - 1, bz = ((o & 4) ? H : 0) + z0 / 2 - 1;
	auto       clampN = [](int c) { return c < 0 ? 0 : (c >= N ? N - 1 : c); };
	for (int base = tid; base < TOT; base += 4 * TPB) {
		double v0[4], v1[4], v2[4], w0[4], w1[4], w2[4];
#pragma unroll
		for (int j = 0; j < 4; j++) {
			const int  idx = base + j * TPB;
			const int  lx = idx % W, ly = (idx / W) % W, lz = idx / WW;
			const int  c[3]   = {bx + lx, by + ly, bz + lz};
			const int  cl[3]  = {clampN(c[0]), clampN(c[1]), clampN(c[2])};
			const bool out[3] = {c[0] != cl[0], c[1] != cl[1], c[2] != cl[2]};
			const int  k      = (int) out[0] + (int) out[1] + (int) out[2];
			const double *p = ep + cl[0] + N * cl[1] + NN * cl[2]; // the cell itself, or m just inside the face
			int           st = 0;                                  // physical face: the step to m1, towards the inside
			if (k == 1 && idx < TOT) {
				const int a    = out[0] ? 0 : (out[1] ? 1 : 2);
				const int upr  = c[a] >= N;
				const int side = 2 * a + upr;
				const int kind = fk[side], src = fs[side];
				const int fa = a == 0 ? cl[1] : cl[0], fb = a == 2 ? cl[1] : cl[2]; // the face's two other axes, in order
				if (kind == FACE_LOCAL) {
					int nb[3] = {cl[0], cl[1], cl[2]};
					nb[a]     = upr ? 0 : N - 1;
					p         = e + (size_t) src * NNN + nb[0] + N * nb[1] + NN * nb[2];
				}
				if (kind == FACE_GHOST) p = C.ghost + (size_t) src * NN + fa + N * fb;
				if (kind == FACE_DIRICHLET || kind == FACE_NEUMANN) {
					const int sa = a == 0 ? 1 : (a == 1 ? N : NN);
					st           = upr ? -sa : sa;
				}
			}
			w0[j] = st ? 3.0 : 1.0, w1[j] = st ? -3.0 : 0.0, w2[j] = st ? 1.0 : 0.0;
			v0[j] = p[0];
			v1[j] = p[st];
			v2[j] = p[2 * st];
		}
#pragma unroll
		for (int j = 0; j < 4; j++)
			if (base + j * TPB < TOT) E[base + j * TPB] = (w0[j] * v0[j] + w1[j] * v1[j]) + w2[j] * v2[j];
	}
	ldsBarrier();
	// edges and corners of the parent that the ring touches: from the face entries (one axis out of range, the others clamped)
	for (int idx = tid; idx < TOT; idx += TPB) {
		const int  lx = idx % W, ly = (idx / W) % W, lz = idx / WW;
		const int  l[3]   = {lx, ly, lz};
		const int  c[3]   = {bx + lx, by + ly, bz + lz};
		const bool out[3] = {c[0] < 0 || c[0] >= N, c[1] < 0 || c[1] >= N, c[2] < 0 || c[2] >= N};
		if ((int) out[0] + (int) out[1] + (int) out[2] < 2) continue;
		int li[3]; // the clamped cell's entry
#pragma unroll
		for (int a = 0; a < 3; a++) li[a] = out[a] ? (c[a] < 0 ? l[a] + 1 : l[a] - 1) : l[a];
		const double m   = E[li[0] + W * li[1] + WW * li[2]];
		double       tot = -2.0 * m;
		tot += out[0] ? E[l[0] + W * li[1] + WW * li[2]] : m;
		tot += out[1] ? E[li[0] + W * l[1] + WW * li[2]] : m;
		tot += out[2] ? E[li[0] + W * li[1] + WW * l[2]] : m;
		E[idx] = tot;
	}
	ldsBarrier();

	// ---- the march: pm, pcur, pn = coarse planes lz - 1, lz, lz + 1 interpolated in x and y: [fine row 2Y | 2Y + 1] as pairs in x
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
			for (int k = 0; k < 2; k++) { // rows 2Y + k of fine planes 2j (towards the plane below) and 2j + 1 (above)
				up2[(2 * j) * NP + q[k]]     = double2{quad3(pcur[k].x, pm[k].x, pn[k].x), quad3(pcur[k].y, pm[k].y, pn[k].y)};
				up2[(2 * j + 1) * NP + q[k]] = double2{quad3(pcur[k].x, pn[k].x, pm[k].x), quad3(pcur[k].y, pn[k].y, pm[k].y)};
			}
		}
	}
}

// E of coarse patch pc at (cx, cy) for the quadratic interpolation (2D: the rule above with two axes)
__device__ __forceinline__ double extendedQuad2d(const Level2D &C, const double *e, int pc, int cx, int cy)
{
	const int     n = C.n;
	const bool    ox = cx < 0 || cx >= n, oy = cy < 0 || cy >= n;
	const int     clx = cx < 0 ? 0 : (cx >= n ? n - 1 : cx), cly = cy < 0 ? 0 : (cy >= n ? n - 1 : cy);
	const double *mp = e + (size_t) pc * n * n + clx + n * cly;
	const double  m  = *mp;
	if (!ox && !oy) return m;
	auto face = [&](int s, int t, int st) { // the ghost through side s: extrapolated on a physical face, the operator's otherwise
		const int kind = C.face_kind[pc * 4 + s];
		if (kind == FACE_DIRICHLET || kind == FACE_NEUMANN) return (3.0 * m - 3.0 * mp[st]) + mp[2 * st];
		return ghost2d(C, e, pc, s, t, m, false);
	};
	const double gx = ox ? face(cx < 0 ? 0 : 1, cly, cx < 0 ? 1 : -1) : m;
	const double gy = oy ? face(cy < 0 ? 2 : 3, clx, cy < 0 ? n : -n) : m;
	if (ox && oy) return (-m + gx) + gy;
	return ox ? gx : gy;
}
static __global__ __launch_bounds__(256) void k_prolong_quadratic2d(Level2D C, int Pf, const int32_t *__restrict__ parent,
                                                                    const int32_t *__restrict__ orth, const double *__restrict__ e,
                                                                    double *__restrict__ u)
{
	const int    n = C.n, h = n / 2;
	const size_t total = (size_t) Pf * n * h;
	for (size_t idx = (size_t) blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t) gridDim.x * blockDim.x) {
		const int pf = (int) (idx / ((size_t) n * h)), q = (int) (idx % ((size_t) n * h));
		const int y = q / h, X = q % h;
		const int o = orth[pf], pc = parent[pf];
		double2  *fp = reinterpret_cast<double2 *>(u + (size_t) pf * n * n + 2 * X + n * y);
		if (o < 0) {
			*fp = *reinterpret_cast<const double2 *>(e + (size_t) pc * n * n + 2 * X + n * y);
			continue;
		}
		const int cx = X + ((o & 1) ? h : 0), cy = (y + ((o & 2) ? n : 0)) >> 1, dy = (y & 1) ? 1 : -1;
		double2   xr[3]; // rows cy, cy + dy, cy - dy
#pragma unroll
		for (int r = 0; r < 3; r++) {
			const int    yy = r == 0 ? cy : (r == 1 ? cy + dy : cy - dy);
			const double a = extendedQuad2d(C, e, pc, cx - 1, yy), b = extendedQuad2d(C, e, pc, cx, yy), c = extendedQuad2d(C, e, pc, cx + 1, yy);
			xr[r] = double2{quad3(b, a, c), quad3(b, c, a)};
		}
		*fp = double2{quad3(xr[0].x, xr[1].x, xr[2].x), quad3(xr[0].y, xr[1].y, xr[2].y)};
	}
}
} // namespace te
