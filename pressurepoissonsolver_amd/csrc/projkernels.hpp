// The operators that turn a pressure into a velocity correction, consistent with the library's own discrete Laplacian: the MAC
// (face-centred) gradient of a cell vector, the divergence of a face vector, and the projection U -= alpha grad p in one pass.
// Nothing in the reference computes these; they exist so that a flow solver's time step stays on the device.
//
// FACE VECTOR (te_vec_create_faces): one normal component per cell face, stored per patch -- a face shared by two patches is stored
// by both. Per patch, D = dim, n = cells per axis, D n^D + D n^(D-1) doubles:
//   LO_a, a = 0..D-1   n^D doubles each, cell layout (x fastest): the component on the LOWER a-face of the cell
//   HI_a, a = 0..D-1   n^(D-1) doubles each, laid out like a ghost slot / boundary block of side 2a+1: the patch's UPPER a-face
// Components are taken ALONG THE AXIS (not along the outward normal).
//
//   gradient    interior face   (u[c] - u[c - e_a]) / h_a
//               patch face      (m - ghost) / h_a below, (ghost - m) / h_a above; ghost = the value the stencil kernels read there
//                               (neighbour cell, ghost slot; Dirichlet: 2 g - m; Neumann: the face carries g_n itself)
//   divergence  out[c] = alpha * sum_a (U_a(upper face of c) - LO_a[c]) / h_a          (patch-local: no ghosts)
//   project     U = fma(-alpha, G, U) with G as above, never stored
// A difference is always formed as upper cell minus lower cell and then multiplied by 1 / h_a: the two copies of a same-level face
// get the same bits, on one rank and across ranks.
//
// 3D: plane marches in the shape of k_stencil3d (march3d.hpp) -- one workgroup per patch or z-slab, a thread owns a 2x2 column,
// planes in a register ring requested two steps ahead, x/y neighbours through the LDS tile, halos through haloSrc / zPlaneSrc with
// a second (pointer, scale) pair for the boundary data. Nothing a step requests is consumed by the same step; every load of the
// loop is unconditional, from a pointer chosen before the loop. 2D: the simple form of k_stencil2d (neighbours from global memory).
//
// Algorithmic bytes per site, n = 32, 3D (a face layer is 1/32 of a patch; 6 halo layers read, 3 HI layers written):
//   gradient    read 8 + 6/32 * 8 = 9.5,   written 3 * 8 + 3/32 * 8 = 24.75            -> 34.25
//   divergence  read 24.75,                written 8                                   -> 32.75
//   project     read 9.5 + 24.75,          written 24.75                               -> 59
#pragma once
#include "march3d.hpp"
#include "kernels2d.hpp"

namespace te
{
struct FaceGeom {
	const double  *h;     // [P][3] spacings
	const int32_t *bface; // [P][2 dim] block of the face in a boundary vector (-1: none); null without boundary data
	const double  *bdata; // boundary vector, or null (homogeneous)
};

// the second term of a halo value: value(z) += s * p[z * stride] (boundary data of a physical face; scale 0 elsewhere)
struct BHaloSrc {
	const double *p;
	int           stride;
	double        s;
};

template <int N, bool PROJECT, int ZS>
__global__ __launch_bounds__(Tile3<N>::TPB) void k_gradient3d(LevelDev L, FaceGeom fg, const double *__restrict__ u, double *G, double alpha)
{
	using T           = Tile3<N>;
	constexpr int TPB = T::TPB, NP = T::NP, H = T::H;
	constexpr int NN = N * N, NNN = N * N * N;
	constexpr int ZL = N / ZS;
	constexpr size_t FV = 3 * (size_t) NNN + 3 * NN;
	const int nblocks = L.count * ZS;
	const int work    = xcdRemap(blockIdx.x, nblocks);
	if (work >= nblocks) return;
	const int pid = L.order ? L.order[L.first + work / ZS] : L.first + work / ZS;
	const int z0  = (work % ZS) * ZL;
	const int tid = threadIdx.x;
	const bool last = z0 + ZL == N;

	__shared__ __attribute__((aligned(16))) double tile[2][T::LSZ];

	const Reg6     fk(L.face_kind + (size_t) pid * 6), fs(L.face_src + (size_t) pid * 6);
	const bool     has_b = fg.bdata != nullptr;
	const Reg6     bf(has_b ? fg.bface + (size_t) pid * 6 : L.face_kind + (size_t) pid * 6);
	const double   ihx = 1.0 / fg.h[(size_t) pid * 3], ihy = 1.0 / fg.h[(size_t) pid * 3 + 1], ihz = 1.0 / fg.h[(size_t) pid * 3 + 2];
	const double  *up  = u + (size_t) pid * NNN;
	const double2 *up2 = reinterpret_cast<const double2 *>(up);
	double        *Gp  = G + (size_t) pid * FV;
	double2       *lo2 = reinterpret_cast<double2 *>(Gp); // LO_a plane z: lo2[a * NNN / 2 + z * NP + q]
	double2       *hi2 = reinterpret_cast<double2 *>(Gp + 3 * (size_t) NNN); // HI_a: hi2[a * NN / 2 + ...]

	const bool act = (T::NT == TPB) || tid < T::NT;
	const int  X = act ? tid % H : 0, Yp = act ? tid / H : 0;
	int        q[2], lds[2];
	const int  ldo[2] = {T::row(2 * Yp) + 2 * X + 2, T::row(2 * Yp + 3) + 2 * X + 2};
#pragma unroll
	for (int k = 0; k < 2; k++) {
		q[k]   = (2 * Yp + k) * H + X;
		lds[k] = T::row(2 * Yp + k + 1) + 2 * X + 2;
	}
	// a Neumann face carries its datum itself: these threads store the halo value instead of a difference
	const bool nW = fk[0] == FACE_NEUMANN && X == 0, nE = fk[1] == FACE_NEUMANN, nS = fk[2] == FACE_NEUMANN && Yp == 0, nN = fk[3] == FACE_NEUMANN;
	const bool nB = fk[4] == FACE_NEUMANN, nT = fk[5] == FACE_NEUMANN;
	const bool east = act && X == H - 1, north = act && Yp == H - 1;

	// halos: Dirichlet ghost = -m + 2 g, Neumann "ghost" = g_n, a neighbour's cell or a ghost slot as it is
	HaloSrc  hs = haloSrc<N>(tid, fk, fs, u, up, L.ghost, -1.0, 0.0, L.xf);
	BHaloSrc hb{up, 0, 0.0};
	if (tid < 4 * N && has_b) {
		const int side = tid / N, t = tid % N, kind = fk[side], b = bf[side];
		if (kind == FACE_DIRICHLET && b >= 0) hb.p = fg.bdata + (size_t) b * NN + t, hb.stride = N, hb.s = 2.0;
		if (kind == FACE_NEUMANN && b >= 0) hs.p = fg.bdata + (size_t) b * NN + t, hs.stride = N, hs.s = 1.0;
	}
	PlaneSrc bot = zPlaneSrc<N>(fk[4], fs[4], false, u, up, L.ghost, -1.0, 0.0);
	PlaneSrc top = zPlaneSrc<N>(fk[5], fs[5], true, u, up, L.ghost, -1.0, 0.0);
	PlaneSrc botb{up2, 0.0}, topb{up2, 0.0};
	if (has_b) {
		if (fk[4] == FACE_DIRICHLET && bf[4] >= 0) botb.p = reinterpret_cast<const double2 *>(fg.bdata + (size_t) bf[4] * NN), botb.s = 2.0;
		if (fk[4] == FACE_NEUMANN && bf[4] >= 0) bot.p = reinterpret_cast<const double2 *>(fg.bdata + (size_t) bf[4] * NN), bot.s = 1.0;
		if (fk[5] == FACE_DIRICHLET && bf[5] >= 0) topb.p = reinterpret_cast<const double2 *>(fg.bdata + (size_t) bf[5] * NN), topb.s = 2.0;
		if (fk[5] == FACE_NEUMANN && bf[5] >= 0) top.p = reinterpret_cast<const double2 *>(fg.bdata + (size_t) bf[5] * NN), top.s = 1.0;
	}
	// PROJECT: where this thread's HI_x / HI_y pairs of U sit (a harmless address and stride 0 for the threads that own none)
	const double2 *hxp = east ? hi2 + Yp : lo2;
	const double2 *hyp = north ? hi2 + NN / 2 + X : lo2;
	const int      hxs = east ? H : 0, hys = north ? H : 0;

	// ---- register pipeline over z: um, uc = planes z-1, z; planes z+1, z+2 in flight in a two-slot ring (plane p in slot p & 1).
	// PROJECT: the three LO planes and the HI_x / HI_y pairs of U for plane z are requested one step ahead.
	double2 um[2], uc[2], ur[2][2];
	double2 Ur[3][2] = {}, Uc[3][2] = {}, Uhx{}, Uhy{}, Uhxc{}, Uhyc{}; // (PROJECT only)
	auto clampP = [&](int p) { return p < N ? p : N - 1; };
	{
		const double2 *pm = z0 == 0 ? bot.p : up2 + (z0 - 1) * NP;
		const double   sm = z0 == 0 ? bot.s : 1.0, sb = z0 == 0 ? botb.s : 0.0;
#pragma unroll
		for (int k = 0; k < 2; k++) {
			const double2 a = pm[q[k]], b = botb.p[q[k]];
			uc[k] = double2{sm * a.x + sb * b.x, sm * a.y + sb * b.y};
		}
	}
	double hraw = hs.p[z0 * hs.stride], braw = hb.p[z0 * hb.stride];
	__builtin_amdgcn_sched_barrier(0);
#pragma unroll
	for (int i = 0; i < 2; i++) {
#pragma unroll
		for (int k = 0; k < 2; k++) ur[i][k] = up2[(z0 + i) * NP + q[k]];
		__builtin_amdgcn_sched_barrier(0);
	}
	if (PROJECT) {
#pragma unroll
		for (int a = 0; a < 3; a++)
#pragma unroll
			for (int k = 0; k < 2; k++) Ur[a][k] = lo2[a * (NNN / 2) + z0 * NP + q[k]];
		Uhx = hxp[z0 * hxs];
		Uhy = hyp[z0 * hys];
		__builtin_amdgcn_sched_barrier(0);
	}
	auto upd = [&](double2 U, double2 g) { // U - alpha g with one rounding, the same on every path
		return PROJECT ? double2{__builtin_fma(-alpha, g.x, U.x), __builtin_fma(-alpha, g.y, U.y)} : g;
	};

	auto step = [&](auto par, auto refill, int zz) {
		constexpr int  PAR    = decltype(par)::value;
		constexpr bool REFILL = decltype(refill)::value;
		const int      z      = z0 + zz;
		const double   hv     = hs.s * takeReg(hraw) + hb.s * takeReg(braw);
		if (REFILL || PAR == 0) {
			hraw = hs.p[clampP(z + 1) * hs.stride];
			braw = hb.p[clampP(z + 1) * hb.stride];
		}
		__builtin_amdgcn_sched_barrier(0);
#pragma unroll
		for (int k = 0; k < 2; k++) {
			um[k] = uc[k];
			uc[k] = takeRegs(ur[PAR][k]);
			if (REFILL) ur[PAR][k] = up2[(z + 2) * NP + q[k]];
		}
		if (PROJECT) {
#pragma unroll
			for (int a = 0; a < 3; a++)
#pragma unroll
				for (int k = 0; k < 2; k++) {
					Uc[a][k] = takeRegs(Ur[a][k]);
					if (REFILL || PAR == 0) Ur[a][k] = lo2[a * (NNN / 2) + clampP(z + 1) * NP + q[k]];
				}
			Uhxc = takeRegs(Uhx);
			Uhyc = takeRegs(Uhy);
			if (REFILL || PAR == 0) {
				Uhx = hxp[clampP(z + 1) * hxs];
				Uhy = hyp[clampP(z + 1) * hys];
			}
		}

		double *tl = tile[PAR];
		if (act) {
			ldsStore2(tl + lds[0], uc[0]);
			ldsStore2(tl + lds[1], uc[1]);
		}
		if (hs.lds >= 0) tl[hs.lds] = hv;
		ldsBarrier();

		const double2 ylo = ldsLoad2(tl + ldo[0]);
		const double2 yhi = ldsLoad2(tl + ldo[1]);
		const bool    zb  = nB && z == 0;
		double        hx[2];
#pragma unroll
		for (int k = 0; k < 2; k++) {
			const double *t0 = tl + lds[k];
			const double2 c  = uc[k];
			const double2 ym = (k == 0) ? ylo : uc[0];
			const double  xl = t0[-1], xr = t0[2];
			double2       gx, gy, gz;
			gx.x = nW ? xl : (c.x - xl) * ihx;
			gx.y = (c.y - c.x) * ihx;
			gy.x = (k == 0 && nS) ? ym.x : (c.x - ym.x) * ihy;
			gy.y = (k == 0 && nS) ? ym.y : (c.y - ym.y) * ihy;
			gz.x = zb ? um[k].x : (c.x - um[k].x) * ihz;
			gz.y = zb ? um[k].y : (c.y - um[k].y) * ihz;
			hx[k] = nE ? xr : (xr - c.y) * ihx;
			if (act) {
				lo2[z * NP + q[k]]                 = upd(Uc[0][k], gx);
				lo2[NNN / 2 + z * NP + q[k]]       = upd(Uc[1][k], gy);
				lo2[2 * (NNN / 2) + z * NP + q[k]] = upd(Uc[2][k], gz);
			}
		}
		if (east) hi2[Yp + H * z] = upd(Uhxc, double2{hx[0], hx[1]}); // HI_x[y + N z], rows 2 Yp and 2 Yp + 1
		if (north) {
			double2 gy;
			gy.x = nN ? yhi.x : (yhi.x - uc[1].x) * ihy;
			gy.y = nN ? yhi.y : (yhi.y - uc[1].y) * ihy;
			hi2[NN / 2 + X + H * z] = upd(Uhyc, gy); // HI_y[x + N z]
		}
	};
	using B0 = std::integral_constant<int, 0>;
	using B1 = std::integral_constant<int, 1>;
	static_assert(ZL % 2 == 0 && ZL >= 4, "the march is unrolled over the two ring slots and ends with two steps of its own");
#pragma unroll 1
	for (int zz = 0; zz < ZL - 2; zz += 2) {
		step(B0{}, std::true_type{}, zz);
		step(B1{}, std::true_type{}, zz + 1);
	}
	// the plane above the patch (and its boundary data, and U's HI_z) is requested two steps before the last slab needs it
	double2 tp[2], tb[2], Ut[2] = {};
#pragma unroll
	for (int k = 0; k < 2; k++) {
		tp[k] = top.p[q[k]];
		tb[k] = topb.p[q[k]];
		if (PROJECT) Ut[k] = hi2[NN + q[k]];
	}
	__builtin_amdgcn_sched_barrier(0);
	step(B0{}, std::false_type{}, ZL - 2);
	step(B1{}, std::false_type{}, ZL - 1);
	if (last && act) {
#pragma unroll
		for (int k = 0; k < 2; k++) {
			const double2 t{top.s * tp[k].x + topb.s * tb[k].x, top.s * tp[k].y + topb.s * tb[k].y};
			double2       gz;
			gz.x = nT ? t.x : (t.x - uc[k].x) * ihz;
			gz.y = nT ? t.y : (t.y - uc[k].y) * ihz;
			hi2[NN + q[k]] = upd(Ut[k], gz); // HI_z[x + N y]
		}
	}
}

// out = alpha div U: reads only its own patch. Upper x-neighbour: the pair's other cell, the next lane's first cell, HI_x on the
// last pair; y: the other row's registers, the next row pair through LDS, HI_y on the last row; z: the register ring, HI_z above
// the last plane. Every plane is requested two steps before the step that uses it.
template <int N, int ZS>
__global__ __launch_bounds__(Tile3<N>::TPB) void k_divergence3d(int P, const double *__restrict__ hgeom, const double *__restrict__ U,
                                                                 double *__restrict__ out, double alpha)
{
	using T           = Tile3<N>;
	constexpr int TPB = T::TPB, NP = T::NP, H = T::H;
	constexpr int NN = N * N, NNN = N * N * N;
	constexpr int ZL = N / ZS;
	constexpr size_t FV = 3 * (size_t) NNN + 3 * NN;
	const int nblocks = P * ZS;
	const int work    = xcdRemap(blockIdx.x, nblocks);
	if (work >= nblocks) return;
	const int pid = work / ZS, z0 = (work % ZS) * ZL, tid = threadIdx.x;

	__shared__ double2 rows[2][TPB + H];

	const double   ihx = 1.0 / hgeom[(size_t) pid * 3], ihy = 1.0 / hgeom[(size_t) pid * 3 + 1], ihz = 1.0 / hgeom[(size_t) pid * 3 + 2];
	const double2 *lo2 = reinterpret_cast<const double2 *>(U + (size_t) pid * FV);
	const double2 *hi2 = reinterpret_cast<const double2 *>(U + (size_t) pid * FV + 3 * (size_t) NNN);
	double2       *op2 = reinterpret_cast<double2 *>(out + (size_t) pid * NNN);
	const bool     act = (T::NT == TPB) || tid < T::NT;
	const int      X = act ? tid % H : 0, Yp = act ? tid / H : 0;
	const int      q[2] = {(2 * Yp) * H + X, (2 * Yp + 1) * H + X};
	const bool     east = X == H - 1, north = Yp == H - 1;
	const double2 *hxp = east ? hi2 + Yp : lo2;
	const double2 *hyp = north ? hi2 + NN / 2 + X : lo2;
	const int      hxs = east ? H : 0, hys = north ? H : 0;
	auto zPlane = [&](int p) { return p < N ? lo2 + 2 * (NNN / 2) + p * NP : hi2 + NN; }; // LO_z plane p, HI_z above the last

	// two-slot rings, plane p in slot p & 1: LO_x, LO_y and this thread's HI_x / HI_y pairs of planes z, z+1; LO_z of planes z+1, z+2
	double2 xs[2][2], ys[2][2], zs[2][2], hxs_[2], hys_[2], zc[2], zn[2];
#pragma unroll
	for (int k = 0; k < 2; k++) zn[k] = zPlane(z0)[q[k]];
	__builtin_amdgcn_sched_barrier(0);
#pragma unroll
	for (int i = 0; i < 2; i++) { // oldest first
#pragma unroll
		for (int k = 0; k < 2; k++) {
			xs[i][k]     = lo2[(z0 + i) * NP + q[k]];
			ys[i][k]     = lo2[NNN / 2 + (z0 + i) * NP + q[k]];
			zs[1 - i][k] = zPlane(z0 + 1 + i)[q[k]];
		}
		hxs_[i] = hxp[(z0 + i) * hxs];
		hys_[i] = hyp[(z0 + i) * hys];
		__builtin_amdgcn_sched_barrier(0);
	}

	auto step = [&](auto par, auto refill, int zz) {
		constexpr int  PAR    = decltype(par)::value; // zz & 1 (z0 is even)
		constexpr bool REFILL = decltype(refill)::value;
		const int      z      = z0 + zz;
		double2        lx[2], ly[2];
		const double2  hx = takeRegs(hxs_[PAR]), hy = takeRegs(hys_[PAR]);
#pragma unroll
		for (int k = 0; k < 2; k++) {
			zc[k] = zn[k];
			zn[k] = takeRegs(zs[1 - PAR][k]); // plane z + 1
			lx[k] = takeRegs(xs[PAR][k]);
			ly[k] = takeRegs(ys[PAR][k]);
		}
		if (REFILL) { // planes z + 2 (z + 3 of LO_z): in the slab, or HI_z above its last plane
#pragma unroll
			for (int k = 0; k < 2; k++) {
				zs[1 - PAR][k] = zPlane(z + 3)[q[k]];
				xs[PAR][k]     = lo2[(z + 2) * NP + q[k]];
				ys[PAR][k]     = lo2[NNN / 2 + (z + 2) * NP + q[k]];
			}
			hxs_[PAR] = hxp[(z + 2) * hxs];
			hys_[PAR] = hyp[(z + 2) * hys];
		}
		rows[PAR][tid] = ly[0];
		ldsBarrier();
		const double2 yn = rows[PAR][tid + H]; // row 2 Yp + 2 (the last row pair reads a slot nobody needs)
		const double2 yu = north ? hy : yn;
		// the next pair's first cell: the next lane (pairs of a row are consecutive lanes; the row's last pair takes HI_x)
		const double nx0 = __shfl_down(lx[0].x, 1), nx1 = __shfl_down(lx[1].x, 1);
		const double xu0 = east ? hx.x : nx0, xu1 = east ? hx.y : nx1;
		double2      r[2];
		r[0].x = (lx[0].y - lx[0].x) * ihx + (ly[1].x - ly[0].x) * ihy + (zn[0].x - zc[0].x) * ihz;
		r[0].y = (xu0 - lx[0].y) * ihx + (ly[1].y - ly[0].y) * ihy + (zn[0].y - zc[0].y) * ihz;
		r[1].x = (lx[1].y - lx[1].x) * ihx + (yu.x - ly[1].x) * ihy + (zn[1].x - zc[1].x) * ihz;
		r[1].y = (xu1 - lx[1].y) * ihx + (yu.y - ly[1].y) * ihy + (zn[1].y - zc[1].y) * ihz;
		if (act) {
			op2[z * NP + q[0]] = double2{alpha * r[0].x, alpha * r[0].y};
			op2[z * NP + q[1]] = double2{alpha * r[1].x, alpha * r[1].y};
		}
	};
	using B0 = std::integral_constant<int, 0>;
	using B1 = std::integral_constant<int, 1>;
	static_assert(ZL % 2 == 0 && ZL >= 4, "two steps per iteration, two steps at the end");
#pragma unroll 1
	for (int zz = 0; zz < ZL - 2; zz += 2) {
		step(B0{}, std::true_type{}, zz);
		step(B1{}, std::true_type{}, zz + 1);
	}
	step(B0{}, std::false_type{}, ZL - 2);
	step(B1{}, std::false_type{}, ZL - 1);
}

// ---- 2D twins, in the simple form of k_stencil2d: one thread per pair of x-adjacent cells, neighbours from global memory.
// Per patch: LO_x n^2, LO_y n^2, HI_x n (by y), HI_y n (by x).
// the gradient on face s of patch p at face coordinate t, m = the cell just inside
__device__ __forceinline__ double faceGrad2d(const Level2D &L, const FaceGeom &fg, const double *u, int p, int s, int t, double m, double ih)
{
	const int    n = L.n, kind = L.face_kind[p * 4 + s];
	const int    b = fg.bdata ? fg.bface[p * 4 + s] : -1;
	const double g = b >= 0 ? fg.bdata[(size_t) b * n + t] : 0.0;
	if (kind == FACE_NEUMANN) return g;
	const double ghost = kind == FACE_DIRICHLET ? 2 * g - m : ghost2d(L, u, p, s, t, m, false);
	return (s & 1) ? (ghost - m) * ih : (m - ghost) * ih;
}
template <bool PROJECT>
__global__ __launch_bounds__(256) void k_gradient2d(Level2D L, FaceGeom fg, const double *__restrict__ u, double *G, double alpha)
{
	const int    n = L.n, h = n / 2;
	const size_t total = (size_t) L.P * n * h, FV = 2 * (size_t) n * n + 2 * n;
	auto         upd = [&](double U, double g) { return PROJECT ? __builtin_fma(-alpha, g, U) : g; };
	for (size_t idx = (size_t) blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t) gridDim.x * blockDim.x) {
		const int     p = (int) (idx / ((size_t) n * h)), q = (int) (idx % ((size_t) n * h));
		const int     y = q / h, x = 2 * (q % h);
		const double *up = u + (size_t) p * n * n;
		double       *Gp = G + (size_t) p * FV;
		const double  ihx = 1.0 / fg.h[(size_t) p * 3], ihy = 1.0 / fg.h[(size_t) p * 3 + 1];
		const double2 c = *reinterpret_cast<const double2 *>(up + x + n * y);
		double2       gx, gy;
		gx.x = (x > 0) ? (c.x - up[x - 1 + n * y]) * ihx : faceGrad2d(L, fg, u, p, 0, y, c.x, ihx);
		gx.y = (c.y - c.x) * ihx;
		if (y > 0) {
			const double2 ym = *reinterpret_cast<const double2 *>(up + x + n * (y - 1));
			gy = double2{(c.x - ym.x) * ihy, (c.y - ym.y) * ihy};
		} else {
			gy = double2{faceGrad2d(L, fg, u, p, 2, x, c.x, ihy), faceGrad2d(L, fg, u, p, 2, x + 1, c.y, ihy)};
		}
		double2 *ox = reinterpret_cast<double2 *>(Gp + x + n * y), *oy = reinterpret_cast<double2 *>(Gp + (size_t) n * n + x + n * y);
		double2  Ux{0, 0}, Uy{0, 0};
		if (PROJECT) Ux = *ox, Uy = *oy;
		*ox = double2{upd(Ux.x, gx.x), upd(Ux.y, gx.y)};
		*oy = double2{upd(Uy.x, gy.x), upd(Uy.y, gy.y)};
		if (x + 2 == n) {
			double *o = Gp + 2 * (size_t) n * n + y;
			*o        = upd(PROJECT ? *o : 0.0, faceGrad2d(L, fg, u, p, 1, y, c.y, ihx));
		}
		if (y == n - 1) {
			double2 *o = reinterpret_cast<double2 *>(Gp + 2 * (size_t) n * n + n + x);
			double2  Uh{0, 0};
			if (PROJECT) Uh = *o;
			*o = double2{upd(Uh.x, faceGrad2d(L, fg, u, p, 3, x, c.x, ihy)), upd(Uh.y, faceGrad2d(L, fg, u, p, 3, x + 1, c.y, ihy))};
		}
	}
}
// (inline: densitykernels.hpp includes this header in a second unit)
inline __global__ __launch_bounds__(256) void k_divergence2d(int P, int n, const double *__restrict__ hgeom, const double *__restrict__ U,
                                                      double *__restrict__ out, double alpha)
{
	const int    h = n / 2;
	const size_t total = (size_t) P * n * h, FV = 2 * (size_t) n * n + 2 * n;
	for (size_t idx = (size_t) blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t) gridDim.x * blockDim.x) {
		const int     p = (int) (idx / ((size_t) n * h)), q = (int) (idx % ((size_t) n * h));
		const int     y = q / h, x = 2 * (q % h);
		const double *lx = U + (size_t) p * FV, *ly = lx + (size_t) n * n, *hx = ly + (size_t) n * n, *hy = hx + n;
		const double  ihx = 1.0 / hgeom[(size_t) p * 3], ihy = 1.0 / hgeom[(size_t) p * 3 + 1];
		const double2 a  = *reinterpret_cast<const double2 *>(lx + x + n * y);
		const double2 b  = *reinterpret_cast<const double2 *>(ly + x + n * y);
		const double  xu = (x + 2 < n) ? lx[x + 2 + n * y] : hx[y];
		const double2 yu = *reinterpret_cast<const double2 *>(y + 1 < n ? ly + x + n * (y + 1) : hy + x);
		double2       r;
		r.x = (a.y - a.x) * ihx + (yu.x - b.x) * ihy;
		r.y = (xu - a.y) * ihx + (yu.y - b.y) * ihy;
		*reinterpret_cast<double2 *>(out + (size_t) p * n * n + x + n * y) = double2{alpha * r.x, alpha * r.y};
	}
}
} // namespace te
