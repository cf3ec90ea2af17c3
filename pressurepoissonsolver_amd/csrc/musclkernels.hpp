// Second-order limited (MUSCL) transport of a cell field by a MAC face velocity: limited slopes of a cell
// field as three cell vectors, and advectkernels.hpp's flux and update with the cell operands replaced by edge states. Nothing in
// the reference computes these. Vector layouts: projkernels.hpp (face vector), bckernels.hpp (boundary vector).
//
//   slope of a cell along axis a    dm = c - m, dp = p - c, with m and p the operands beyond the cell's lower and upper a-face: the
//                                   same-level neighbour's facing cell; on a physical face the boundary vector's entry, or without
//                                   cb the cell itself; the covering coarse cell, raw, where the neighbour is coarser; the average
//                                   of the covering fine cells where the neighbours are finer (k_cf_raw3d / k_cf_raw2d's slots)
//     TE_SLOPE_ZERO (0)      S = 0.0
//     TE_SLOPE_MINMOD (1)    S = (dm*dp > 0.0) ? (fabs(dm) < fabs(dp) ? dm : dp) : 0.0
//     TE_SLOPE_MC (2)        t = 0.5*(dm + dp), w = fmin(fmin(2.0*fabs(dm), 2.0*fabs(dp)), fabs(t)), S = (dm*dp > 0.0) ? copysign(w, dm) : 0.0
//     TE_SLOPE_CENTRAL (3)   S = 0.5*(dm + dp)     (unlimited: no positivity guarantee)
//   flux of a face                  upwindFlux (s = (U >= 0.0) ? lo : hi, F = U * s) with the cell operands replaced by edge states:
//                                   a cell on the lower side of the face contributes lo = c + 0.5*S_a, a cell on the upper side
//                                   hi = c - 0.5*S_a; an operand that is not a cell of this level (the boundary datum, the own cell
//                                   standing in for it, the raw coarse cell, the coarse cell on the coarse side) enters as it is
//     same-level interior face      both sides are edge states; the two patches' copies get the same bits when U's copies agree
//     coarse/fine face, fine side   upwindFlux(U_f, C, m - 0.5*S) on a lower face, upwindFlux(U_f, m + 0.5*S, C) on an upper one
//     coarse/fine face, coarse side faceMean4 / faceMean2 of those fine-side values, formed from the fine patch's own U, m, S and
//                                   this C: the coarse copy IS the mean of the fine copies; the coarse copy of U is never read
//   The scheme is first order at coarse/fine and physical faces and second order elsewhere.
//
// Every operation is rounded on its own: FMA contraction is off for this file, the fma's of the divergence are explicit (divPart).
//
// 3D. k_slopes3d<N, ZS>: k_cellface3d's march (one workgroup per patch or z-slab, a thread owns a 2x2 column, x/y neighbours through
// the LDS tile) with three planes in registers (z - 1, z, z + 1) and planes z + 2, z + 3 in flight: a step consumes a plane two
// steps after it was requested. c is read once, the three slope planes are written.
// advectMusclMarch<N, ZS, FUSED>: advectMarch with the thread's own S_x, S_y, S_z pairs streamed beside c and U (a set in use, the
// next plane's set in flight, requested a whole step ahead). S_x and S_y go through LDS tiles of their own beside c's, so that the
// x-neighbour's S_x and the row below's / above's S_y are read where the neighbouring cell is read; the halo entries of these
// tiles come from a haloSrc on the S_a vector and are used on a same-level side only. The plane below's upper edge state is carried
// in registers; below and above a slab stand the next slab's S_z planes or, on a same-level side, the neighbour's (zPlaneSrc).
// Every z-slab count gives the one-slab bits: the operands and the expressions are the same.
//
// Algorithmic bytes per site, n = 32, 3D (a cell layer is 1/32 of a patch, a face vector 24.75 B per site):
//   cell_slopes          read 8 + 6/32 * 8 = 9.5,                                  written 24            -> 33.5
//   advect_flux_muscl    the slopes, then read 9.5 + 24.75 (U) + 3 * (8 + 2/32 * 8) = 25.5 (S), written 24.75 -> 33.5 + 84.5 = 118
//   advect_muscl         the slopes, then read 9.5 + 24.75 + 25.5,                  written 8             -> 33.5 + 67.75 = 101.25
#pragma once
#include "densitykernels.hpp" // k_cf_raw3d / k_cf_raw2d
#include "advectkernels.hpp"  // upwindFlux, divPart (and FMA contraction is off from there to the end of the unit)

namespace te
{
#pragma clang fp contract(off)

enum SlopeKind : int { SLOPE_ZERO = 0, SLOPE_MINMOD = 1, SLOPE_MC = 2, SLOPE_CENTRAL = 3 };

__device__ __forceinline__ double cellSlope(int kind, double dm, double dp)
{
	if (kind == SLOPE_ZERO) return 0.0;
	const double t = 0.5 * (dm + dp);
	if (kind == SLOPE_CENTRAL) return t;
	const double am = fabs(dm), ap = fabs(dp);
	const double w  = (kind == SLOPE_MINMOD) ? (am < ap ? dm : dp) : copysign(fmin(fmin(2.0 * am, 2.0 * ap), fabs(t)), dm);
	return (dm * dp > 0.0) ? w : 0.0;
}
__device__ __forceinline__ double2 cellSlope2(int kind, double2 m, double2 c, double2 p)
{
	return double2{cellSlope(kind, c.x - m.x, p.x - c.x), cellSlope(kind, c.y - m.y, p.y - c.y)};
}
// the edge states of a cell: what it contributes to its upper (c + 0.5 S) and to its lower (c - 0.5 S) face along S's axis
__device__ __forceinline__ double edgeUp(double c, double S) { return c + 0.5 * S; }
__device__ __forceinline__ double edgeLo(double c, double S) { return c - 0.5 * S; }
__device__ __forceinline__ double2 edgeUp2(double2 c, double2 S) { return double2{edgeUp(c.x, S.x), edgeUp(c.y, S.y)}; }
__device__ __forceinline__ double2 edgeLo2(double2 c, double2 S) { return double2{edgeLo(c.x, S.x), edgeLo(c.y, S.y)}; }

// The slopes of c along x, y, z. The halo value of a side is k_cellface3d's: a neighbour's cell, a ghost slot (k_cf_raw3d), the
// boundary vector's entry or the own cell.
template <int N, int ZS>
__global__ __launch_bounds__(Tile3<N>::TPB) void k_slopes3d(LevelDev L, FaceGeom fg, const double *__restrict__ c, double *__restrict__ sx,
                                                             double *__restrict__ sy, double *__restrict__ sz, int kind)
{
	using T           = Tile3<N>;
	constexpr int TPB = T::TPB, NP = T::NP, H = T::H;
	constexpr int NN = N * N, NNN = N * N * N;
	constexpr int ZL = N / ZS;
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
	const double  *cp  = c + (size_t) pid * NNN;
	const double2 *cp2 = reinterpret_cast<const double2 *>(cp);
	double2       *sx2 = reinterpret_cast<double2 *>(sx + (size_t) pid * NNN);
	double2       *sy2 = reinterpret_cast<double2 *>(sy + (size_t) pid * NNN);
	double2       *sz2 = reinterpret_cast<double2 *>(sz + (size_t) pid * NNN);

	const bool act = (T::NT == TPB) || tid < T::NT;
	const int  X = act ? tid % H : 0, Yp = act ? tid / H : 0;
	int        q[2], lds[2];
	const int  ldo[2] = {T::row(2 * Yp) + 2 * X + 2, T::row(2 * Yp + 3) + 2 * X + 2};
#pragma unroll
	for (int k = 0; k < 2; k++) {
		q[k]   = (2 * Yp + k) * H + X;
		lds[k] = T::row(2 * Yp + k + 1) + 2 * X + 2;
	}
	auto phys = [](int kd) { return kd == FACE_DIRICHLET || kd == FACE_NEUMANN; };

	// halos, all taken as they are: a neighbour's cell, a ghost slot, the boundary vector's entry or the own cell
	HaloSrc hs = haloSrc<N>(tid, fk, fs, c, cp, L.ghost, 1.0, 1.0);
	if (tid < 4 * N && has_b) {
		const int side = tid / N, t = tid % N, b = bf[side];
		if (phys(fk[side]) && b >= 0) hs.p = fg.bdata + (size_t) b * NN + t, hs.stride = N;
	}
	PlaneSrc bot = zPlaneSrc<N>(fk[4], fs[4], false, c, cp, L.ghost, 1.0, 1.0);
	PlaneSrc top = zPlaneSrc<N>(fk[5], fs[5], true, c, cp, L.ghost, 1.0, 1.0);
	if (has_b) {
		if (phys(fk[4]) && bf[4] >= 0) bot.p = reinterpret_cast<const double2 *>(fg.bdata + (size_t) bf[4] * NN);
		if (phys(fk[5]) && bf[5] >= 0) top.p = reinterpret_cast<const double2 *>(fg.bdata + (size_t) bf[5] * NN);
	}
	const double2 *ctop = last ? top.p : cp2 + (z0 + ZL) * NP; // the plane above the slab

	// ---- register pipeline over z: um, uc, un = planes z-1, z, z+1; planes z+2, z+3 in flight in a two-slot ring (plane p in slot p & 1)
	double2 um[2], uc[2], un[2], ur[2][2];
	auto clampP = [&](int p) { return p < N ? p : N - 1; };
	{
		const double2 *pm = z0 == 0 ? bot.p : cp2 + (z0 - 1) * NP;
#pragma unroll
		for (int k = 0; k < 2; k++) uc[k] = pm[q[k]];
	}
	double hraw = hs.p[z0 * hs.stride];
	__builtin_amdgcn_sched_barrier(0);
#pragma unroll
	for (int k = 0; k < 2; k++) un[k] = cp2[z0 * NP + q[k]];
	__builtin_amdgcn_sched_barrier(0);
#pragma unroll
	for (int i = 1; i <= 2; i++) {
#pragma unroll
		for (int k = 0; k < 2; k++) ur[i & 1][k] = cp2[(z0 + i) * NP + q[k]];
		__builtin_amdgcn_sched_barrier(0);
	}

	// REFILL: 0 plane z + 3 of the slab, 1 the plane above the slab, 2 nothing
	auto step = [&](auto par, auto refill, int zz) {
		constexpr int PAR    = decltype(par)::value;
		constexpr int REFILL = decltype(refill)::value;
		const int     z      = z0 + zz;
		const double  hv     = takeReg(hraw);
		if (REFILL < 2 || PAR == 0) hraw = hs.p[clampP(z + 1) * hs.stride];
		__builtin_amdgcn_sched_barrier(0);
#pragma unroll
		for (int k = 0; k < 2; k++) {
			um[k] = uc[k];
			uc[k] = un[k];
			un[k] = takeRegs(ur[1 - PAR][k]); // plane z + 1
			if (REFILL == 0) ur[1 - PAR][k] = cp2[(z + 3) * NP + q[k]];
			if (REFILL == 1) ur[1 - PAR][k] = ctop[q[k]];
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
#pragma unroll
		for (int k = 0; k < 2; k++) {
			const double *t0 = tl + lds[k];
			const double2 v  = uc[k];
			const double2 ym = (k == 0) ? ylo : uc[0], yp = (k == 0) ? uc[1] : yhi;
			const double  xl = t0[-1], xr = t0[2];
			if (act) {
				sx2[z * NP + q[k]] = double2{cellSlope(kind, v.x - xl, v.y - v.x), cellSlope(kind, v.y - v.x, xr - v.y)};
				sy2[z * NP + q[k]] = cellSlope2(kind, ym, v, yp);
				sz2[z * NP + q[k]] = cellSlope2(kind, um[k], v, un[k]);
			}
		}
	};
	using B0 = std::integral_constant<int, 0>;
	using B1 = std::integral_constant<int, 1>;
	using B2 = std::integral_constant<int, 2>;
	static_assert(ZL % 2 == 0 && ZL >= 4, "the march is unrolled over the two ring slots and ends with four steps of its own");
#pragma unroll 1
	for (int zz = 0; zz < ZL - 4; zz += 2) {
		step(B0{}, B0{}, zz);
		step(B1{}, B0{}, zz + 1);
	}
	step(B0{}, B0{}, ZL - 4); // requests the slab's last plane
	step(B1{}, B1{}, ZL - 3); // ... the plane above it
	step(B0{}, B2{}, ZL - 2);
	step(B1{}, B2{}, ZL - 1);
}

// Ghost slots of the coarse/fine faces for te_advect_flux_muscl / te_advect_muscl: the face's flux, k_cf_flux3d with the fine cell's
// edge state in the place of the fine cell. S[ax] is the slope vector along the face's axis.
template <int N>
__global__ void k_cf_flux_muscl3d(const int32_t *__restrict__ desc, const int32_t *__restrict__ slots, const double *__restrict__ U,
                                  const double *__restrict__ c, const double *__restrict__ sx, const double *__restrict__ sy,
                                  const double *__restrict__ sz, double *__restrict__ ghost)
{
	constexpr int    NN = N * N, NNN = N * N * N;
	constexpr size_t FV = 3 * (size_t) NNN + 3 * NN;
	const int32_t   *d = desc + (size_t) blockIdx.x * 8;
	const int        p = d[0], s = d[1], kind = d[2], q = d[3];
	const int        ax = s >> 1, up = s & 1;
	const int        sa = (ax == 0) ? N : 1, sb = (ax == 2) ? N : NN, sn = (ax == 0) ? 1 : (ax == 1 ? N : NN);
	const int        mine = up ? (N - 1) * sn : 0, oth = up ? 0 : (N - 1) * sn; // my face layer, the neighbour's facing layer
	double          *g  = ghost + (size_t) slots[blockIdx.x] * NN;
	const double    *S  = ax == 0 ? sx : (ax == 1 ? sy : sz);
	const double    *cm = c + (size_t) p * NNN + mine, *Sm = S + (size_t) p * NNN + mine;
	// patch r's stored entry of its lower (upper = 0) or upper a-face at face point (a, b)
	auto faceU = [&](int r, int upper, int a, int b) {
		const double *Ur = U + (size_t) r * FV;
		return upper ? Ur[3 * (size_t) NNN + ax * NN + a + N * b] : Ur[(size_t) ax * NNN + a * sa + b * sb];
	};
	for (int i = threadIdx.x; i < NN; i += blockDim.x) {
		const int    a = i % N, b = i / N;
		const double m = cm[a * sa + b * sb];
		if (kind == 2) { // I am the fine patch: my cell's edge state against the raw coarse cell
			const int ca = (a + ((q & 1) ? N : 0)) / 2, cb = (b + ((q & 2) ? N : 0)) / 2;
			if (d[4] < 0) continue;
			const double C = c[(size_t) d[4] * NNN + oth + ca * sa + cb * sb], Uf = faceU(p, up, a, b), Sv = Sm[a * sa + b * sb];
			g[i]           = up ? upwindFlux(Uf, edgeUp(m, Sv), C) : upwindFlux(Uf, C, edgeLo(m, Sv));
		} else { // I am the coarse patch: my raw cell against the fine cells' edge states (the fine patch's side is s ^ 1)
			const int qa = (a >= N / 2), qb = (b >= N / 2);
			const int nbq = d[4 + qa + 2 * qb];
			const int fa = 2 * (a - qa * (N / 2)), fb = 2 * (b - qb * (N / 2));
			if (nbq < 0) continue;
			const size_t  fo = (size_t) nbq * NNN + oth + fa * sa + fb * sb;
			const double *f = c + fo, *Sf = S + fo;
			double        F[2][2]; // [along a][along b]
#pragma unroll
			for (int bb = 0; bb < 2; bb++)
#pragma unroll
				for (int aa = 0; aa < 2; aa++) {
					const double Uf = faceU(nbq, !up, fa + aa, fb + bb), fc = f[aa * sa + bb * sb], Sv = Sf[aa * sa + bb * sb];
					F[aa][bb]       = up ? upwindFlux(Uf, m, edgeLo(fc, Sv)) : upwindFlux(Uf, edgeUp(fc, Sv), m);
				}
			g[i] = faceMean4(F[0][0], F[1][0], F[0][1], F[1][1]);
		}
	}
}

// The march of te_advect_flux_muscl (FUSED = false: out is the face vector F) and of te_advect_muscl (FUSED = true: out is the cell
// vector): a copy of advectMarch, extended by the slope streams (see the head of this file).
template <int N, int ZS, bool FUSED>
__device__ __forceinline__ void advectMusclMarch(const LevelDev &L, const FaceGeom &fg, const double *__restrict__ c, const double *__restrict__ U,
                                                 const double *__restrict__ sx, const double *__restrict__ sy, const double *__restrict__ sz,
                                                 double *__restrict__ out, double alpha)
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

	__shared__ __attribute__((aligned(16))) double tile[3][2][T::LSZ]; // c, S_x, S_y

	const Reg6     fk(L.face_kind + (size_t) pid * 6), fs(L.face_src + (size_t) pid * 6);
	const bool     has_b = fg.bdata != nullptr;
	const Reg6     bf(has_b ? fg.bface + (size_t) pid * 6 : L.face_kind + (size_t) pid * 6);
	const double   ihx = 1.0 / fg.h[(size_t) pid * 3], ihy = 1.0 / fg.h[(size_t) pid * 3 + 1], ihz = 1.0 / fg.h[(size_t) pid * 3 + 2];
	const double  *cp  = c + (size_t) pid * NNN;
	const double2 *cp2 = reinterpret_cast<const double2 *>(cp);
	const double  *sp[3] = {sx + (size_t) pid * NNN, sy + (size_t) pid * NNN, sz + (size_t) pid * NNN};
	const double2 *sp2[3] = {reinterpret_cast<const double2 *>(sp[0]), reinterpret_cast<const double2 *>(sp[1]), reinterpret_cast<const double2 *>(sp[2])};
	const double2 *ulo = reinterpret_cast<const double2 *>(U + (size_t) pid * FV); // LO_a plane z: ulo[a * NNN / 2 + z * NP + q]
	const double2 *uhi = reinterpret_cast<const double2 *>(U + (size_t) pid * FV + 3 * (size_t) NNN);
	double2       *lo2 = reinterpret_cast<double2 *>(out + (size_t) pid * FV);                     // (FUSED = false)
	double2       *hi2 = reinterpret_cast<double2 *>(out + (size_t) pid * FV + 3 * (size_t) NNN); // (FUSED = false)
	double2       *op2 = reinterpret_cast<double2 *>(out + (size_t) pid * NNN);                    // (FUSED = true)

	const bool act = (T::NT == TPB) || tid < T::NT;
	const int  X = act ? tid % H : 0, Yp = act ? tid / H : 0;
	int        q[2], lds[2];
	const int  ldo[2] = {T::row(2 * Yp) + 2 * X + 2, T::row(2 * Yp + 3) + 2 * X + 2};
#pragma unroll
	for (int k = 0; k < 2; k++) {
		q[k]   = (2 * Yp + k) * H + X;
		lds[k] = T::row(2 * Yp + k + 1) + 2 * X + 2;
	}
	auto phys = [](int kd) { return kd == FACE_DIRICHLET || kd == FACE_NEUMANN; };
	// on a coarse/fine side the halo value is the face's flux itself (k_cf_flux_muscl3d), everywhere else the operand beyond the face
	const bool gW = fk[0] == FACE_GHOST && X == 0, gE = fk[1] == FACE_GHOST, gS = fk[2] == FACE_GHOST && Yp == 0,
	           gN = fk[3] == FACE_GHOST && Yp == H - 1;
	const bool gB = fk[4] == FACE_GHOST, gT = fk[5] == FACE_GHOST && last;
	// is the operand beyond the column's west / east / south / north / bottom / top face a cell of this level (it enters by its edge state)?
	const bool eW = X > 0 || fk[0] == FACE_LOCAL, eE = fk[1] == FACE_LOCAL, eS = Yp > 0 || fk[2] == FACE_LOCAL,
	           eN = Yp < H - 1 || fk[3] == FACE_LOCAL;
	const bool eB = z0 > 0 || fk[4] == FACE_LOCAL, eT = !last || fk[5] == FACE_LOCAL;
	const bool east = act && X == H - 1, north = act && Yp == H - 1;

	// halos of c, all taken as they are: a neighbour's cell, a ghost slot, the boundary vector's entry or the own cell
	HaloSrc hs = haloSrc<N>(tid, fk, fs, c, cp, L.ghost, 1.0, 1.0);
	if (tid < 4 * N && has_b) {
		const int side = tid / N, t = tid % N, b = bf[side];
		if (phys(fk[side]) && b >= 0) hs.p = fg.bdata + (size_t) b * NN + t, hs.stride = N;
	}
	// halos of the slopes: S_x beyond the west / east side, S_y beyond the south / north side -- the neighbour's facing layer on a
	// same-level side; on every other side some readable value that nobody uses (eW .. eN)
	const int     hax = (tid < 2 * N) ? 0 : 1;
	const HaloSrc hss = haloSrc<N>(tid, fk, fs, hax == 0 ? sx : sy, hax == 0 ? sp[0] : sp[1], L.ghost, 1.0, 1.0);
	const int     hsl = (1 + hax) * 2 * T::LSZ + hss.lds; // its place in tile[1 + hax][0]
	PlaneSrc bot = zPlaneSrc<N>(fk[4], fs[4], false, c, cp, L.ghost, 1.0, 1.0);
	PlaneSrc top = zPlaneSrc<N>(fk[5], fs[5], true, c, cp, L.ghost, 1.0, 1.0);
	if (has_b) {
		if (phys(fk[4]) && bf[4] >= 0) bot.p = reinterpret_cast<const double2 *>(fg.bdata + (size_t) bf[4] * NN);
		if (phys(fk[5]) && bf[5] >= 0) top.p = reinterpret_cast<const double2 *>(fg.bdata + (size_t) bf[5] * NN);
	}
	const PlaneSrc sbot = zPlaneSrc<N>(fk[4], fs[4], false, sz, sp[2], L.ghost, 1.0, 1.0);
	const PlaneSrc stop = zPlaneSrc<N>(fk[5], fs[5], true, sz, sp[2], L.ghost, 1.0, 1.0);
	// the plane above the slab, its S_z and U on the faces below it: the next slab's first plane and its LO_z, or the plane above the patch and HI_z
	const double2 *ctop = last ? top.p : cp2 + (z0 + ZL) * NP;
	const double2 *sztop = last ? stop.p : sp2[2] + (z0 + ZL) * NP;
	const double2 *utop = last ? uhi + NN : ulo + 2 * (NNN / 2) + (z0 + ZL) * NP;
	// where this thread's HI_x pair sits (the threads that own none: entry 0, stride 0, of LO), and U_y above its column: LO_y of row
	// 2 Yp + 2 or, on the last row pair, HI_y (FUSED = false needs it there only)
	const double2 *Uhxp = east ? uhi + Yp : ulo, *Uyup = north ? uhi + NN / 2 + X : (FUSED ? ulo + NNN / 2 + q[1] + H : ulo);
	const int      hxs = east ? H : 0, uys = north ? H : (FUSED ? NP : 0);

	// ---- register pipeline over z: um, uc = planes z-1, z; planes z+1, z+2 in flight in a two-slot ring (plane p in slot p & 1).
	// Sc = the slopes of plane z, Sn = those of plane z+1, requested at the start of step z. uze = the upper z edge state of plane
	// z-1 (or the raw operand below the patch). Ul, Uhx, Uyu: U of the plane the NEXT step works on, requested by the step before,
	// behind its fluxes.
	double2 um[2], uc[2], ur[2][2];
	double2 Sc[3][2], Sn[3][2], uze[2];
	double2 Ul[3][2], Uhx, Uyu;
	double2 pt[2] = {}, pfz[2] = {}; // (FUSED) the x/y part of the divergence and the lower z fluxes of the plane one step back
	auto clampP = [&](int p) { return p < N ? p : N - 1; };
	{
		const double2 *pm = z0 == 0 ? bot.p : cp2 + (z0 - 1) * NP;
		const double2 *sm = z0 == 0 ? sbot.p : sp2[2] + (z0 - 1) * NP;
#pragma unroll
		for (int k = 0; k < 2; k++) {
			uc[k]  = pm[q[k]];
			uze[k] = sm[q[k]];
		}
	}
	double hraw = hs.p[z0 * hs.stride], sraw = hss.p[z0 * hss.stride];
	__builtin_amdgcn_sched_barrier(0);
#pragma unroll
	for (int i = 0; i < 2; i++) {
#pragma unroll
		for (int k = 0; k < 2; k++) ur[i][k] = cp2[(z0 + i) * NP + q[k]];
		__builtin_amdgcn_sched_barrier(0);
	}
	auto requestS = [&](int z) { // the slopes of plane z
#pragma unroll
		for (int a = 0; a < 3; a++)
#pragma unroll
			for (int k = 0; k < 2; k++) Sn[a][k] = sp2[a][z * NP + q[k]];
	};
	auto request = [&](int z) { // U of plane z
#pragma unroll
		for (int a = 0; a < 3; a++)
#pragma unroll
			for (int k = 0; k < 2; k++) Ul[a][k] = ulo[a * (NNN / 2) + z * NP + q[k]];
		Uhx = Uhxp[z * hxs];
		Uyu = Uyup[z * uys];
	};
	requestS(z0);
	__builtin_amdgcn_sched_barrier(0);
	request(z0);
	__builtin_amdgcn_sched_barrier(0);
#pragma unroll
	for (int k = 0; k < 2; k++) uze[k] = eB ? edgeUp2(uc[k], uze[k]) : uc[k];
	// (FUSED) plane zp = c - alpha * div, the upper z fluxes fzu given
	auto finish = [&](int zp, const double2 *cc, const double2 *fzu) {
#pragma unroll
		for (int k = 0; k < 2; k++) {
			const double rx = __builtin_fma(fzu[k].x - pfz[k].x, ihz, pt[k].x), ry = __builtin_fma(fzu[k].y - pfz[k].y, ihz, pt[k].y);
			const double dx = alpha * rx, dy = alpha * ry;
			if (act) op2[zp * NP + q[k]] = double2{cc[k].x - dx, cc[k].y - dy};
		}
	};

	auto step = [&](auto par, auto refill, auto more, int zz) {
		constexpr int  PAR    = decltype(par)::value;
		constexpr bool REFILL = decltype(refill)::value;
		constexpr bool MORE   = decltype(more)::value; // another step of this slab follows
		const int      z      = z0 + zz;
		const double   hv = takeReg(hraw), sv = takeReg(sraw);
		if (REFILL || PAR == 0) {
			hraw = hs.p[clampP(z + 1) * hs.stride];
			sraw = hss.p[clampP(z + 1) * hss.stride];
		}
		__builtin_amdgcn_sched_barrier(0);
#pragma unroll
		for (int k = 0; k < 2; k++) {
			um[k] = uc[k];
			uc[k] = takeRegs(ur[PAR][k]);
			if (REFILL) ur[PAR][k] = cp2[(z + 2) * NP + q[k]];
		}
#pragma unroll
		for (int a = 0; a < 3; a++)
#pragma unroll
			for (int k = 0; k < 2; k++) Sc[a][k] = takeRegs(Sn[a][k]);
		__builtin_amdgcn_sched_barrier(0);
		if (MORE) requestS(z + 1);
		__builtin_amdgcn_sched_barrier(0);

		double *tl = tile[0][PAR], *tx = tile[1][PAR], *ty = tile[2][PAR];
		if (act) {
#pragma unroll
			for (int k = 0; k < 2; k++) {
				ldsStore2(tl + lds[k], uc[k]);
				ldsStore2(tx + lds[k], Sc[0][k]);
				ldsStore2(ty + lds[k], Sc[1][k]);
			}
		}
		if (hs.lds >= 0) {
			tl[hs.lds]                           = hv;
			(&tile[0][0][0])[hsl + PAR * T::LSZ] = sv;
		}
		ldsBarrier();

		const double2 ylo = ldsLoad2(tl + ldo[0]), yhi = ldsLoad2(tl + ldo[1]);
		const double2 sylo = ldsLoad2(ty + ldo[0]), syhi = ldsLoad2(ty + ldo[1]);
		const bool    zb  = gB && z == 0;
		double2       fx[2], fy[2], fz[2], yup[2], zlo[2];
		double        hx[2];
#pragma unroll
		for (int k = 0; k < 2; k++) {
			const double2 v   = uc[k];
			const double2 xlo = edgeLo2(v, Sc[0][k]), xup = edgeUp2(v, Sc[0][k]); // the cells' own edge states
			const double2 yl  = edgeLo2(v, Sc[1][k]);
			yup[k]            = edgeUp2(v, Sc[1][k]);
			zlo[k]            = edgeLo2(v, Sc[2][k]);
			const double xl = tl[lds[k] - 1], xr = tl[lds[k] + 2], sxl = tx[lds[k] - 1], sxr = tx[lds[k] + 2];
			const double xle = eW ? edgeUp(xl, sxl) : xl, xre = eE ? edgeLo(xr, sxr) : xr;
			const double2 ybl = (k == 0) ? (eS ? edgeUp2(ylo, sylo) : ylo) : yup[0]; // what stands below the row
			fx[k].x = gW ? xl : upwindFlux(Ul[0][k].x, xle, xlo.x);
			fx[k].y = upwindFlux(Ul[0][k].y, xup.x, xlo.y);
			fy[k]   = (k == 0 && gS) ? ylo : upwindFlux2(Ul[1][k], ybl, yl);
			fz[k]   = zb ? um[k] : upwindFlux2(Ul[2][k], uze[k], zlo[k]);
			hx[k]   = gE ? xr : upwindFlux(k == 0 ? Uhx.x : Uhx.y, xup.y, xre);
		}
		const double2 fyu = gN ? yhi : upwindFlux2(Uyu, yup[1], eN ? edgeLo2(yhi, syhi) : yhi); // the y faces above the column
#pragma unroll
		for (int k = 0; k < 2; k++) uze[k] = edgeUp2(uc[k], Sc[2][k]); // what this plane contributes to the z faces above it
		// this plane's U is consumed: the next plane's into the same registers, one step ahead of its use
		__builtin_amdgcn_sched_barrier(0);
		if (MORE) request(z + 1);
		__builtin_amdgcn_sched_barrier(0);
		if (!FUSED) {
#pragma unroll
			for (int k = 0; k < 2; k++)
				if (act) {
					lo2[z * NP + q[k]]                 = fx[k];
					lo2[NNN / 2 + z * NP + q[k]]       = fy[k];
					lo2[2 * (NNN / 2) + z * NP + q[k]] = fz[k];
				}
			if (east) hi2[Yp + H * z] = double2{hx[0], hx[1]}; // HI_x[y + N z], rows 2 Yp and 2 Yp + 1
			if (north) hi2[NN / 2 + X + H * z] = fyu;          // HI_y[x + N z]
		} else {
			if (zz > 0) finish(z - 1, um, fz);
			// the next pair's lower x flux: the next lane (pairs of a row are consecutive lanes; the row's last pair takes HI_x)
			const double nx0 = __shfl_down(fx[0].x, 1), nx1 = __shfl_down(fx[1].x, 1);
			const double xu0 = east ? hx[0] : nx0, xu1 = east ? hx[1] : nx1;
			pt[0].x = divPart<false>(fx[0].y - fx[0].x, fy[1].x - fy[0].x, ihx, ihy);
			pt[0].y = divPart<true>(xu0 - fx[0].y, fy[1].y - fy[0].y, ihx, ihy);
			pt[1].x = divPart<false>(fx[1].y - fx[1].x, fyu.x - fy[1].x, ihx, ihy);
			pt[1].y = divPart<(N >= 16)>(xu1 - fx[1].y, fyu.y - fy[1].y, ihx, ihy);
			pfz[0] = fz[0], pfz[1] = fz[1];
		}
	};
	using B0 = std::integral_constant<int, 0>;
	using B1 = std::integral_constant<int, 1>;
	static_assert(ZL % 2 == 0 && ZL >= 4, "the march is unrolled over the two ring slots and ends with two steps of its own");
#pragma unroll 1
	for (int zz = 0; zz < ZL - 2; zz += 2) {
		step(B0{}, std::true_type{}, std::true_type{}, zz);
		step(B1{}, std::true_type{}, std::true_type{}, zz + 1);
	}
	// the plane above the slab, its S_z and U below it are requested two steps before the last plane needs them
	double2 tp[2], Ut[2], St[2];
#pragma unroll
	for (int k = 0; k < 2; k++) {
		tp[k] = ctop[q[k]];
		St[k] = sztop[q[k]];
		Ut[k] = utop[q[k]];
	}
	__builtin_amdgcn_sched_barrier(0);
	step(B0{}, std::false_type{}, std::true_type{}, ZL - 2);
	step(B1{}, std::false_type{}, std::false_type{}, ZL - 1);
	double2 ft[2];
#pragma unroll
	for (int k = 0; k < 2; k++) ft[k] = gT ? tp[k] : upwindFlux2(Ut[k], uze[k], eT ? edgeLo2(tp[k], St[k]) : tp[k]);
	if (FUSED) {
		finish(z0 + ZL - 1, uc, ft);
	} else if (last && act) {
#pragma unroll
		for (int k = 0; k < 2; k++) hi2[NN + q[k]] = ft[k]; // HI_z[x + N y]
	}
}

template <int N, int ZS>
__global__ __launch_bounds__(Tile3<N>::TPB) void k_advflux_muscl3d(LevelDev L, FaceGeom fg, const double *__restrict__ c, const double *__restrict__ U,
                                                                    const double *__restrict__ sx, const double *__restrict__ sy,
                                                                    const double *__restrict__ sz, double *__restrict__ F)
{
	advectMusclMarch<N, ZS, false>(L, fg, c, U, sx, sy, sz, F, 0.0);
}
template <int N, int ZS>
__global__ __launch_bounds__(Tile3<N>::TPB) void k_advect_muscl3d(LevelDev L, FaceGeom fg, const double *__restrict__ c, const double *__restrict__ U,
                                                                   const double *__restrict__ sx, const double *__restrict__ sy,
                                                                   const double *__restrict__ sz, double *__restrict__ out, double alpha)
{
	advectMusclMarch<N, ZS, true>(L, fg, c, U, sx, sy, sz, out, alpha);
}

// ---- 2D twins, in the simple form of k_cellface2d / k_advect2d: one thread per pair of x-adjacent cells, neighbours from global memory.
// the operand beyond side s of patch p at face coordinate t, m = the cell just inside: faceCell2d's
__device__ __forceinline__ double beyond2d(const Level2D &L, const FaceGeom &fg, const double *c, int p, int s, int t, double m)
{
	const int n = L.n, kind = L.face_kind[p * 4 + s];
	if (kind == FACE_DIRICHLET || kind == FACE_NEUMANN) {
		const int b = fg.bdata ? fg.bface[p * 4 + s] : -1;
		return b >= 0 ? fg.bdata[(size_t) b * n + t] : m;
	}
	return ghost2d(L, c, p, s, t, m, false); // the neighbour's cell or the ghost slot (k_cf_raw2d)
}
static __global__ __launch_bounds__(256) void k_slopes2d(Level2D L, FaceGeom fg, const double *__restrict__ c, double *__restrict__ sx,
                                                  double *__restrict__ sy, int kind)
{
	const int    n = L.n, h = n / 2, nn = n * n;
	const size_t total = (size_t) L.P * n * h;
	for (size_t idx = (size_t) blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t) gridDim.x * blockDim.x) {
		const int     p = (int) (idx / ((size_t) n * h)), q = (int) (idx % ((size_t) n * h));
		const int     y = q / h, x = 2 * (q % h);
		const double *cp = c + (size_t) p * nn;
		const double2 v  = *reinterpret_cast<const double2 *>(cp + x + n * y);
		const double  xl = (x > 0) ? cp[x - 1 + n * y] : beyond2d(L, fg, c, p, 0, y, v.x);
		const double  xr = (x + 2 < n) ? cp[x + 2 + n * y] : beyond2d(L, fg, c, p, 1, y, v.y);
		double2       ym, yp;
		if (y > 0)
			ym = *reinterpret_cast<const double2 *>(cp + x + n * (y - 1));
		else
			ym = double2{beyond2d(L, fg, c, p, 2, x, v.x), beyond2d(L, fg, c, p, 2, x + 1, v.y)};
		if (y < n - 1)
			yp = *reinterpret_cast<const double2 *>(cp + x + n * (y + 1));
		else
			yp = double2{beyond2d(L, fg, c, p, 3, x, v.x), beyond2d(L, fg, c, p, 3, x + 1, v.y)};
		const size_t at = (size_t) p * nn + x + n * y;
		*reinterpret_cast<double2 *>(sx + at) = double2{cellSlope(kind, v.x - xl, v.y - v.x), cellSlope(kind, v.y - v.x, xr - v.y)};
		*reinterpret_cast<double2 *>(sy + at) = cellSlope2(kind, ym, v, yp);
	}
}

// k_cf_flux2d with the fine cell's edge state in the place of the fine cell
static __global__ void k_cf_flux_muscl2d(int n, const int32_t *__restrict__ desc, const int32_t *__restrict__ slots, const double *__restrict__ U,
                                         const double *__restrict__ c, const double *__restrict__ sx, const double *__restrict__ sy,
                                         double *__restrict__ ghost)
{
	const int32_t *d = desc + (size_t) blockIdx.x * 8;
	const int      p = d[0], s = d[1], kind = d[2], q = d[3];
	const int      ax = s >> 1, up = s & 1, nn = n * n;
	const size_t   FV = 2 * (size_t) nn + 2 * n;
	const int      sa = (ax == 0) ? n : 1, sn = (ax == 0) ? 1 : n;
	const int      mine = up ? (n - 1) * sn : 0, oth = up ? 0 : (n - 1) * sn;
	const double  *S = ax == 0 ? sx : sy;
	double        *g = ghost + (size_t) slots[blockIdx.x] * n;
	auto faceU = [&](int r, int upper, int a) {
		const double *Ur = U + (size_t) r * FV;
		return upper ? Ur[2 * (size_t) nn + ax * n + a] : Ur[(size_t) ax * nn + a * sa];
	};
	for (int a = threadIdx.x; a < n; a += blockDim.x) {
		const double m = c[(size_t) p * nn + mine + a * sa];
		if (kind == 2) {
			const int ca = (a + (q ? n : 0)) / 2;
			if (d[4] < 0) continue;
			const double C = c[(size_t) d[4] * nn + oth + ca * sa], Uf = faceU(p, up, a), Sv = S[(size_t) p * nn + mine + a * sa];
			g[a]           = up ? upwindFlux(Uf, edgeUp(m, Sv), C) : upwindFlux(Uf, C, edgeLo(m, Sv));
		} else {
			const int qa = (a >= n / 2), nbq = d[4 + qa];
			const int fa = 2 * (a - qa * (n / 2));
			if (nbq < 0) continue;
			const size_t fo = (size_t) nbq * nn + oth + fa * sa;
			double       F[2];
#pragma unroll
			for (int aa = 0; aa < 2; aa++) {
				const double Uf = faceU(nbq, !up, fa + aa), fc = c[fo + aa * sa], Sv = S[fo + aa * sa];
				F[aa]           = up ? upwindFlux(Uf, m, edgeLo(fc, Sv)) : upwindFlux(Uf, edgeUp(fc, Sv), m);
			}
			g[a] = faceMean2(F[0], F[1]);
		}
	}
}

// the flux through side s of patch p at face coordinate t: m = the cell just inside, me = its edge state on that face, Uf = the
// patch's stored entry of the face, S = the slope vector along the side's axis
__device__ __forceinline__ double sideFluxMuscl2d(const Level2D &L, const FaceGeom &fg, const double *c, const double *S, int p, int s, int t,
                                                  double m, double me, double Uf)
{
	const int n = L.n, kind = L.face_kind[p * 4 + s], src = L.face_src[p * 4 + s];
	if (kind == FACE_GHOST) return L.ghost[(size_t) src * n + t]; // (k_cf_flux_muscl2d)
	double o;
	if (kind == FACE_DIRICHLET || kind == FACE_NEUMANN) {
		const int b = fg.bdata ? fg.bface[p * 4 + s] : -1;
		o           = b >= 0 ? fg.bdata[(size_t) b * n + t] : m;
	} else {
		const int    cell = s == 0 ? (n - 1) + n * t : (s == 1 ? n * t : (s == 2 ? t + n * (n - 1) : t));
		const size_t at   = (size_t) src * n * n + cell;
		o                 = (s & 1) ? edgeLo(c[at], S[at]) : edgeUp(c[at], S[at]);
	}
	return (s & 1) ? upwindFlux(Uf, me, o) : upwindFlux(Uf, o, me);
}
template <bool FUSED>
__global__ __launch_bounds__(256) void k_advect_muscl2d(Level2D L, FaceGeom fg, const double *__restrict__ c, const double *__restrict__ U,
                                                        const double *__restrict__ sx, const double *__restrict__ sy, double *__restrict__ out,
                                                        double alpha)
{
	const int    n = L.n, h = n / 2, nn = n * n;
	const size_t total = (size_t) L.P * n * h, FV = 2 * (size_t) nn + 2 * n;
	for (size_t idx = (size_t) blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t) gridDim.x * blockDim.x) {
		const int     p = (int) (idx / ((size_t) n * h)), q = (int) (idx % ((size_t) n * h));
		const int     y = q / h, x = 2 * (q % h);
		const double *cp = c + (size_t) p * nn, *sxp = sx + (size_t) p * nn, *syp = sy + (size_t) p * nn;
		const double *ux = U + (size_t) p * FV, *uy = ux + nn, *uhx = uy + nn, *uhy = uhx + n;
		const int     at = x + n * y;
		const double2 v  = *reinterpret_cast<const double2 *>(cp + at);
		const double2 Sx = *reinterpret_cast<const double2 *>(sxp + at), Sy = *reinterpret_cast<const double2 *>(syp + at);
		const double2 Ux = *reinterpret_cast<const double2 *>(ux + at), Uy = *reinterpret_cast<const double2 *>(uy + at);
		const double2 xlo = edgeLo2(v, Sx), xup = edgeUp2(v, Sx), ylo = edgeLo2(v, Sy), yup = edgeUp2(v, Sy); // the cells' own edge states
		double2       fx, fy;
		fx.x = (x > 0) ? upwindFlux(Ux.x, edgeUp(cp[at - 1], sxp[at - 1]), xlo.x) : sideFluxMuscl2d(L, fg, c, sx, p, 0, y, v.x, xlo.x, Ux.x);
		fx.y = upwindFlux(Ux.y, xup.x, xlo.y);
		if (y > 0)
			fy = upwindFlux2(Uy, edgeUp2(*reinterpret_cast<const double2 *>(cp + at - n), *reinterpret_cast<const double2 *>(syp + at - n)), ylo);
		else
			fy = double2{sideFluxMuscl2d(L, fg, c, sy, p, 2, x, v.x, ylo.x, Uy.x), sideFluxMuscl2d(L, fg, c, sy, p, 2, x + 1, v.y, ylo.y, Uy.y)};
		// the faces above the pair: of the patch (HI_x, HI_y) or of the next cells
		const bool xe = x + 2 == n, ye = y == n - 1;
		double     xu = 0.0;
		double2    yu{0.0, 0.0};
		if (xe) xu = sideFluxMuscl2d(L, fg, c, sx, p, 1, y, v.y, xup.y, uhx[y]);
		if (ye) {
			const double2 Uh = *reinterpret_cast<const double2 *>(uhy + x);
			yu = double2{sideFluxMuscl2d(L, fg, c, sy, p, 3, x, v.x, yup.x, Uh.x), sideFluxMuscl2d(L, fg, c, sy, p, 3, x + 1, v.y, yup.y, Uh.y)};
		}
		if (!FUSED) {
			double *Fp = out + (size_t) p * FV;
			*reinterpret_cast<double2 *>(Fp + at)      = fx;
			*reinterpret_cast<double2 *>(Fp + nn + at) = fy;
			if (xe) Fp[2 * (size_t) nn + y] = xu;
			if (ye) *reinterpret_cast<double2 *>(Fp + 2 * (size_t) nn + n + x) = yu;
		} else {
			if (!xe) xu = upwindFlux(ux[at + 2], xup.y, edgeLo(cp[at + 2], sxp[at + 2]));
			if (!ye)
				yu = upwindFlux2(*reinterpret_cast<const double2 *>(uy + at + n), yup,
				                 edgeLo2(*reinterpret_cast<const double2 *>(cp + at + n), *reinterpret_cast<const double2 *>(syp + at + n)));
			const double ihx = 1.0 / fg.h[(size_t) p * 3], ihy = 1.0 / fg.h[(size_t) p * 3 + 1];
			// k_divergence2d's value as the compiler contracts it: the y product rounded, the x product fused
			const double rx = divPart<false>(fx.y - fx.x, yu.x - fy.x, ihx, ihy), ry = divPart<false>(xu - fx.y, yu.y - fy.y, ihx, ihy);
			const double dx = alpha * rx, dy = alpha * ry;
			*reinterpret_cast<double2 *>(out + (size_t) p * nn + at) = double2{v.x - dx, v.y - dy};
		}
	}
}
} // namespace te
