// The transfer of a level-0 FACE vector (projkernels.hpp: per patch LO_a, a = 0..D-1, then HI_a) from one mesh to the next,
// te_faces_regrid: what te_vec_regrid is for a cell vector, with a refinement that keeps every fine cell's
// te_divergence equal to its coarse cell's. Nothing in the reference does this. The map is te_vec_regrid's (regridkernels.hpp: one
// row of RG_ROW int32 per DESTINATION patch, kind / orthant / source patches).
//
// F_a(i; t) = component a on face plane i = 0 .. n along a at tangential cell indices t: LO_a for i < n, HI_a for i = n.
//   RG_COPY     the source patch's D n^D + D n^(D-1) doubles, bit for bit.
//   RG_COARSEN  coarse face (a, I, t) = the mean of the 2^(D-1) fine faces that cover it, in the child with orthant bits
//               o_a = (I >= n/2), o_b = (t_b >= n/2): fine plane 2I - o_a n (the mid-plane is the upper child's plane 0), fine
//               tangential indices 2 t_b - o_b n + {0, 1}. 3D: ((p00 + p10) + (p01 + p11)) * 0.25, first index along the lower
//               remaining axis; 2D: (p0 + p1) * 0.5 -- te_boundary_restrict's associations.
//   RG_REFINE   the patch is orthant o of source patch X, h = X's spacings. For b != a
//                 s_ab(i; t) = (F_a(i; t + e_b) - F_a(i; t - e_b)) * 0.125,
//               F_a extended along b by F(-1) = (3 F(0) - 3 F(1)) + F(2), F(n) = (3 F(n-1) - 3 F(n-2)) + F(n-3): every patch edge is
//               one-sided, no ghost of the source hierarchy is read. Fine plane i_f = 0 .. n and fine tangential indices t_f map to
//               X's doubled lattice, I = i_f + o_a n, T_b = t_b + o_b n, c_b = T_b >> 1, sigma_b = -1 (T_b even) / +1 (odd), and
//                 G_a(i; T) = F_a(i; c) + sum_{b != a, ascending} sigma_b s_ab(i; c)
//                 I even:  G_a(I / 2; T)
//                 I odd:   c_a = (I - 1) / 2,
//                          0.5 (G_a(c_a; T) + G_a(c_a + 1; T)) + sum_{b != a, ascending} (0.5 h_a / h_b) (s_ba(c_b + 1; c) - s_ba(c_b; c))
//               The last term is one value per coarse cell and pair (a, b): the difference, between the cell's upper and lower
//               b-face, of component b's slope along a. With it the 2^D fine cells of a coarse cell all have the coarse cell's
//               divergence; fields linear in x, y, z are reproduced; the two copies of a shared face get the same bits (a face's
//               value depends on data of its own plane only, through the same expressions).
// FMA contraction is switched off for this file: the sums above are evaluated exactly as written, on every path.
//
// 3D, k_facexfer3d<N, ZS>: one workgroup per destination patch or z-slab of it (the slab rule of the stencil kernels), so every entry
// has one writer and the kind is uniform per workgroup. Copy and coarsen move double2. Refine works one component at a time: the
// block of F_a over the octant -- H + 1 planes along a, H + 2 entries along each tangential axis (the slab's share along z), at most
// (H + 1)(H + 2)^2 doubles, H = N / 2 -- is staged in LDS in batches of four loads, the tangential ghost entries are extrapolated
// from the entries already there, and thread (X, Y) marches over the coarse cells of its column: ten LDS reads and, for the two
// correction terms, up to twelve global loads (requested one step ahead) give the 24 fine values of a coarse cell and component,
// stored as double2. 2D, k_facexfer2d: one thread per pair of cells, everything from global memory.
// Algorithmic bytes per destination site at N = 32 (a cell, its three lower faces and its share of the HI blocks: 24 + 24/N = 24.75 B):
// copy 49.5; refine 24.75 written and about 4 read (3 of the octant, 4.03 with the rings: 3 x 8 x 17 x 18 x 18 / 32^3); coarsen 24.75
// written and 99 read. The same figures as DESIGN.md section 17 and tools/regrid_time.py.
#pragma once
#include "regridkernels.hpp"

namespace te
{
// In force from here to the end of the translation unit: this header must be the LAST include of the unit that uses it
// (gmg_faceregrid.hip), or whatever is compiled after it silently loses FMA contraction as well.
#pragma clang fp contract(off)

// F(-1) from F(0), F(1), F(2) (or F(n) from F(n-1), F(n-2), F(n-3)), evaluated as written
__device__ __forceinline__ double faceExtrap(double m, double m1, double m2) { return (3.0 * m - 3.0 * m1) + m2; }

// entries first .. first + count of a patch's block as double2, four loads in flight per thread
template <int TPB> __device__ __forceinline__ void copyPairs(double2 *__restrict__ d2, const double2 *__restrict__ e2, int first, int count, int tid)
{
	for (int base = tid; base < count; base += 4 * TPB) {
		const int     i0 = base, i1 = base + TPB, i2 = base + 2 * TPB, i3 = base + 3 * TPB;
		const double2 b0 = e2[first + i0], b1 = e2[first + (i1 < count ? i1 : 0)], b2 = e2[first + (i2 < count ? i2 : 0)],
		              b3 = e2[first + (i3 < count ? i3 : 0)];
		d2[first + i0] = b0;
		if (i1 < count) d2[first + i1] = b1;
		if (i2 < count) d2[first + i2] = b2;
		if (i3 < count) d2[first + i3] = b3;
	}
}

// offset of F_comp at coarse indices (cx, cy, cz) inside a patch's block; the index along comp may be N (HI_comp)
template <int N> __device__ __forceinline__ int faceOff(int comp, int cx, int cy, int cz)
{
	constexpr int NN = N * N, NNN = N * N * N;
	if (comp == 0) return cx < N ? cx + N * cy + NN * cz : 3 * NNN + cy + N * cz;
	if (comp == 1) return cy < N ? NNN + cx + N * cy + NN * cz : 3 * NNN + NN + cx + N * cz;
	return cz < N ? 2 * NNN + cx + N * cy + NN * cz : 3 * NNN + 2 * NN + cx + N * cy;
}

// THE mean of the fine faces that cover a coarse face, for every kernel that coarsens a face vector (the transfer between two meshes
// here, the restriction of the coefficient and its packed form for parents on other ranks in coefkernels.hpp): p[i][j] = the fine
// face at offset i along the lower and j along the higher remaining axis. One place, so the association cannot drift.
__device__ __forceinline__ double faceMean4(double p00, double p10, double p01, double p11) { return ((p00 + p10) + (p01 + p11)) * 0.25; }
__device__ __forceinline__ double faceMean2(double p0, double p1) { return (p0 + p1) * 0.5; }

// a pair of coarse faces whose lower remaining axis runs fastest in memory: q = the first fine face of the first one, s2 = the
// stride of the other remaining axis
__device__ __forceinline__ double2 coarsenPairT(const double *q, int s2)
{
	const double2 a = *reinterpret_cast<const double2 *>(q), b = *reinterpret_cast<const double2 *>(q + 2);
	const double2 c = *reinterpret_cast<const double2 *>(q + s2), d = *reinterpret_cast<const double2 *>(q + s2 + 2);
	return double2{faceMean4(a.x, a.y, c.x, c.y), faceMean4(b.x, b.y, d.x, d.y)};
}
// LO_x: the pair lies along the normal (fine planes q, q + 2), the remaining axes are y (stride N) and z (stride NN)
template <int N> __device__ __forceinline__ double2 coarsenPairX(const double *q)
{
	constexpr int NN = N * N;
	return double2{faceMean4(q[0], q[N], q[NN], q[N + NN]), faceMean4(q[2], q[N + 2], q[NN + 2], q[N + NN + 2])};
}

// the three values a one-sided central difference along an axis needs at index c of 0 .. N-1: (c - 1, c + 1) inside, the three
// entries at the edge otherwise
template <int N> __device__ __forceinline__ void slopeIdx(int c, int *i)
{
	i[0] = c == 0 ? 0 : (c == N - 1 ? N - 1 : c - 1);
	i[1] = c == 0 ? 1 : (c == N - 1 ? N - 2 : c + 1);
	i[2] = c == 0 ? 2 : (c == N - 1 ? N - 3 : c + 1);
}
template <int N> __device__ __forceinline__ double slopeOf(int c, double v0, double v1, double v2)
{
	const double e  = faceExtrap(v0, v1, v2);
	const double up = c == N - 1 ? e : v1, dn = c == 0 ? e : (c == N - 1 ? v1 : v0);
	return (up - dn) * 0.125;
}

template <int N, int ZS>
__global__ __launch_bounds__(Tile3<N>::TPB) void k_facexfer3d(int Pd, const int32_t *__restrict__ map, const double *__restrict__ hsrc,
                                                               const double *__restrict__ src, double *__restrict__ dst)
{
	using T           = Tile3<N>;
	constexpr int TPB = T::TPB, H = T::H, NP = T::NP;
	constexpr int NN = N * N, NNN = N * N * N;
	constexpr size_t FV = 3 * (size_t) NNN + 3 * NN;
	constexpr int ZL = N / ZS; // destination planes of a slab
	constexpr int CZ = ZL / 2; // coarse planes under them (refine)
	constexpr int TOT = (H + 2) * ((H + 1) * (CZ + 2) > (H + 2) * (CZ + 1) ? (H + 1) * (CZ + 2) : (H + 2) * (CZ + 1));
	static_assert(ZL % 2 == 0 && ZL >= 4 && N >= 4, "whole coarse planes, and three entries inside every edge");
	const int nblocks = Pd * ZS;
	const int work    = xcdRemap(blockIdx.x, nblocks);
	if (work >= nblocks) return;
	const int      pd = work / ZS, z0 = (work % ZS) * ZL, tid = threadIdx.x;
	const bool     last = z0 + ZL == N;
	const int32_t *row = map + (size_t) pd * RG_ROW;
	const int      kind = row[0], o = row[1];
	double        *dp = dst + (size_t) pd * FV;
	double2       *lo2 = reinterpret_cast<double2 *>(dp);                    // LO_a plane z: lo2[a * NNN / 2 + z * NP + pair]
	double2       *hi2 = reinterpret_cast<double2 *>(dp + 3 * (size_t) NNN); // HI_a: hi2[a * NN / 2 + ...]

	if (kind == RG_COPY) {
		const double2 *e2 = reinterpret_cast<const double2 *>(src + (size_t) row[2] * FV);
#pragma unroll
		for (int a = 0; a < 3; a++) copyPairs<TPB>(lo2, e2, a * (NNN / 2) + z0 * NP, ZL * NP, tid);
		copyPairs<TPB>(lo2, e2, 3 * (NNN / 2) + z0 * H, ZL * H, tid);          // HI_x[y + N z]
		copyPairs<TPB>(lo2, e2, 3 * (NNN / 2) + NN / 2 + z0 * H, ZL * H, tid); // HI_y[x + N z]
		if (last) copyPairs<TPB>(lo2, e2, 3 * (NNN / 2) + NN, NN / 2, tid);    // HI_z[x + N y]
		return;
	}
	if (kind == RG_COARSEN) { // a pair of coarse faces per thread and step: both lie in one child (N / 2 is even)
		auto child = [&](int ox, int oy, int oz) { return src + (size_t) row[2 + ox + 2 * oy + 4 * oz] * FV; };
		for (int i = tid; i < ZL * NP; i += TPB) {
			const int x = 2 * (i % H), y = (i / H) % N, z = z0 + i / NP;
			const int ox = x >= H, oy = y >= H, oz = z >= H;
			const double *q = child(ox, oy, oz) + (2 * x - ox * N) + N * (2 * y - oy * N) + NN * (2 * z - oz * N);
			lo2[z0 * NP + i]                 = coarsenPairX<N>(q);
			lo2[NNN / 2 + z0 * NP + i]       = coarsenPairT(q + NNN, NN);
			lo2[2 * (NNN / 2) + z0 * NP + i] = coarsenPairT(q + 2 * NNN, N);
		}
		for (int i = tid; i < ZL * H; i += TPB) { // HI_x by (y, z) and HI_y by (x, z): the upper children's HI blocks
			const int t = 2 * (i % H), z = z0 + i / H;
			const int ot = t >= H, oz = z >= H;
			const int f = (2 * t - ot * N) + N * (2 * z - oz * N);
			hi2[z0 * H + i]          = coarsenPairT(child(1, ot, oz) + 3 * NNN + f, N);
			hi2[NN / 2 + z0 * H + i] = coarsenPairT(child(ot, 1, oz) + 3 * NNN + NN + f, N);
		}
		if (last)
			for (int i = tid; i < NP; i += TPB) {
				const int x = 2 * (i % H), y = i / H;
				const int ox = x >= H, oy = y >= H;
				hi2[NN + i] = coarsenPairT(child(ox, oy, 1) + 3 * NNN + 2 * NN + (2 * x - ox * N) + N * (2 * y - oy * N), N);
			}
		return;
	}

	// ---- RG_REFINE
	__shared__ double E[TOT];
	const double *ep = src + (size_t) row[2] * FV;
	const double  hs[3] = {hsrc[(size_t) row[2] * 3], hsrc[(size_t) row[2] * 3 + 1], hsrc[(size_t) row[2] * 3 + 2]};
	const bool    act = (T::NT == TPB) || tid < T::NT;
	const int     X = act ? tid % H : 0, Y = act ? tid / H : 0;
	const int     oc[3] = {(o & 1) ? H : 0, (o & 2) ? H : 0, ((o & 4) ? H : 0) + z0 / 2}; // the slab's first coarse cell in X
	auto          inside = [](int c) { return c >= 0 && c < N; };

	auto component = [&](auto comp) {
		constexpr int A = decltype(comp)::value, B1 = A == 0 ? 1 : 0, B2 = A == 2 ? 1 : 2; // the tangential axes, ascending
		constexpr int RX = A == 0 ? 0 : 1, RY = A == 1 ? 0 : 1, RZ = A == 2 ? 0 : 1;       // ring below the first entry
		constexpr int EX = H + 1 + RX, EY = H + 1 + RY, EZ = CZ + 1 + RZ, EXY = EX * EY, ETOT = EXY * EZ;
		constexpr int SA = A == 0 ? 1 : (A == 1 ? EX : EXY), S1 = B1 == 0 ? 1 : EX, S2 = B2 == 1 ? EX : EXY;
		static_assert(ETOT <= TOT, "the block of a component fits the array");
		const int bx = oc[0] - RX, by = oc[1] - RY, bz = oc[2] - RZ; // entry (lx, ly, lz) is F_A at (bx + lx, by + ly, bz + lz)

		ldsBarrier(); // (the previous component's march has read E)
		for (int base = tid; base < ETOT; base += 4 * TPB) {
			double v[4];
			bool   in[4];
#pragma unroll
			for (int j = 0; j < 4; j++) {
				const int idx = base + j * TPB;
				const int c0 = bx + idx % EX, c1 = by + (idx / EX) % EY, c2 = bz + idx / EXY;
				// (along A every index 0 .. N is a plane; the tangential ones outside the patch are extrapolated below)
				in[j] = idx < ETOT && (A == 0 || inside(c0)) && (A == 1 || inside(c1)) && (A == 2 || inside(c2));
				v[j]  = ep[in[j] ? faceOff<N>(A, c0, c1, c2) : 0];
			}
#pragma unroll
			for (int j = 0; j < 4; j++)
				if (in[j]) E[base + j * TPB] = v[j];
		}
		ldsBarrier();
		// tangential ghosts: the octant touches one face of X per axis (the slab: per z face, or none); entries whose other tangential
		// index is outside too are needed by nobody
		auto ghosts = [&](int lb, int d, int eu, int su, int ev, int sv, int cu0, bool u_tangential, int cv0, bool v_tangential) {
			for (int i = tid; i < eu * ev; i += TPB) {
				const int lu = i % eu, lv = i / eu;
				if ((u_tangential && !inside(cu0 + lu)) || (v_tangential && !inside(cv0 + lv))) continue;
				double *e = E + lb + su * lu + sv * lv;
				e[0]      = faceExtrap(e[d], e[2 * d], e[3 * d]);
			}
		};
		if (A != 0) ghosts((o & 1) ? EX - 1 : 0, (o & 1) ? -1 : 1, EY, EX, EZ, EXY, by, A != 1, bz, A != 2);
		if (A != 1) ghosts(((o & 2) ? EY - 1 : 0) * EX, (o & 2) ? -EX : EX, EX, 1, EZ, EXY, bx, A != 0, bz, A != 2);
		if (A != 2) {
			const bool lo = bz < 0, hi = bz + EZ - 1 >= N;
			if (lo || hi) ghosts((lo ? 0 : EZ - 1) * EXY, lo ? EXY : -EXY, EX, 1, EY, EX, bx, A != 0, by, A != 1);
		}
		ldsBarrier();

		// ---- the march over the coarse cells (X, Y, j) of this thread's column
		const double r1 = 0.5 * (hs[A] / hs[B1]), r2 = 0.5 * (hs[A] / hs[B2]);
		// the correction terms' 12 values of coarse cell j: for b = B1, B2 and b-plane c_b, c_b + 1, F_b at three indices along A
		auto request = [&](int j, double *k) {
			int c[3] = {oc[0] + X, oc[1] + Y, oc[2] + j}, ia[3];
			slopeIdx<N>(c[A], ia);
#pragma unroll
			for (int bb = 0; bb < 2; bb++) {
				const int b = bb == 0 ? B1 : B2;
#pragma unroll
				for (int up = 0; up < 2; up++)
#pragma unroll
					for (int m = 0; m < 3; m++) {
						int q[3] = {c[0], c[1], c[2]};
						q[b] += up, q[A] = ia[m];
						k[6 * bb + 3 * up + m] = ep[faceOff<N>(b, q[0], q[1], q[2])];
					}
			}
		};
		double kn[12], kc[12];
		request(0, kn);
#pragma unroll 1
		for (int j = 0; j < CZ; j++) {
#pragma unroll
			for (int m = 0; m < 12; m++) kc[m] = kn[m];
			request(j + 1 < CZ ? j + 1 : j, kn);
			const int     cA = oc[A] + (A == 0 ? X : (A == 1 ? Y : j));
			const double *e = E + (X + RX) + EX * (Y + RY) + EXY * (j + RZ);
			double        G[2][2][2]; // [plane c_a / c_a + 1][sigma_B1][sigma_B2]
#pragma unroll
			for (int pl = 0; pl < 2; pl++) {
				const double *f = e + pl * SA;
				const double  s1 = (f[S1] - f[-S1]) * 0.125, s2 = (f[S2] - f[-S2]) * 0.125, c = f[0];
				G[pl][0][0] = (c - s1) - s2, G[pl][1][0] = (c + s1) - s2;
				G[pl][0][1] = (c - s1) + s2, G[pl][1][1] = (c + s1) + s2;
			}
			const double k1 = r1 * (slopeOf<N>(cA, kc[3], kc[4], kc[5]) - slopeOf<N>(cA, kc[0], kc[1], kc[2]));
			const double k2 = r2 * (slopeOf<N>(cA, kc[9], kc[10], kc[11]) - slopeOf<N>(cA, kc[6], kc[7], kc[8]));
			double       M[2][2];
#pragma unroll
			for (int u = 0; u < 2; u++)
#pragma unroll
				for (int v = 0; v < 2; v++) M[u][v] = (0.5 * (G[0][u][v] + G[1][u][v]) + k1) + k2;
			if (!act) continue;
			double2 *out = lo2 + A * (NNN / 2) + (z0 + 2 * j) * NP + (2 * Y) * H + X; // fine plane z0 + 2j, row 2Y, pair X
			if (A == 0) {
#pragma unroll
				for (int ky = 0; ky < 2; ky++)
#pragma unroll
					for (int kz = 0; kz < 2; kz++) out[kz * NP + ky * H] = double2{G[0][ky][kz], M[ky][kz]};
				if (X == H - 1)
#pragma unroll
					for (int kz = 0; kz < 2; kz++) hi2[Y + H * (z0 + 2 * j + kz)] = double2{G[1][0][kz], G[1][1][kz]}; // HI_x[y + N z]
			} else if (A == 1) {
#pragma unroll
				for (int kz = 0; kz < 2; kz++) {
					out[kz * NP]     = double2{G[0][0][kz], G[0][1][kz]};
					out[kz * NP + H] = double2{M[0][kz], M[1][kz]};
				}
				if (Y == H - 1)
#pragma unroll
					for (int kz = 0; kz < 2; kz++) hi2[NN / 2 + X + H * (z0 + 2 * j + kz)] = double2{G[1][0][kz], G[1][1][kz]}; // HI_y[x + N z]
			} else {
#pragma unroll
				for (int ky = 0; ky < 2; ky++) {
					out[ky * H]      = double2{G[0][0][ky], G[0][1][ky]};
					out[NP + ky * H] = double2{M[0][ky], M[1][ky]};
				}
				if (last && j == CZ - 1)
#pragma unroll
					for (int ky = 0; ky < 2; ky++) hi2[NN + (2 * Y + ky) * H + X] = double2{G[1][0][ky], G[1][1][ky]}; // HI_z[x + N y]
			}
		}
	};
	component(std::integral_constant<int, 0>{});
	component(std::integral_constant<int, 1>{});
	component(std::integral_constant<int, 2>{});
}

// ---- 2D, the simple form: per patch LO_x n^2, LO_y n^2, HI_x n (by y), HI_y n (by x); everything from global memory
__device__ __forceinline__ double face2d(const double *e, int n, int a, int i, int t)
{
	if (a == 0) return i < n ? e[i + n * t] : e[2 * n * n + t];
	return i < n ? e[n * n + t + n * i] : e[2 * n * n + n + t];
}
// s_ab(i; t), b the other axis
__device__ __forceinline__ double slope2d(const double *e, int n, int a, int i, int t)
{
	auto f = [&](int tt) { return face2d(e, n, a, i, tt); };
	const double up = t == n - 1 ? faceExtrap(f(n - 1), f(n - 2), f(n - 3)) : f(t + 1);
	const double dn = t == 0 ? faceExtrap(f(0), f(1), f(2)) : f(t - 1);
	return (up - dn) * 0.125;
}
__device__ __forceinline__ double refineFace2d(const double *e, int n, const double *h, int o, int a, int i_f, int t_f)
{
	const int b = 1 - a;
	const int I = i_f + ((o >> a) & 1) * n, Tb = t_f + ((o >> b) & 1) * n, cb = Tb >> 1;
	auto      G = [&](int i) {
		const double s = slope2d(e, n, a, i, cb), f = face2d(e, n, a, i, cb);
		return (Tb & 1) ? f + s : f - s;
	};
	if ((I & 1) == 0) return G(I >> 1);
	const int ca = (I - 1) >> 1;
	return 0.5 * (G(ca) + G(ca + 1)) + (0.5 * (h[a] / h[b])) * (slope2d(e, n, b, cb + 1, ca) - slope2d(e, n, b, cb, ca));
}
__device__ __forceinline__ double coarsenFace2d(const double *src, size_t FV, const int32_t *row, int n, int a, int I, int t)
{
	const int     h = n / 2, oa = I >= h, ob = t >= h;
	const double *e = src + (size_t) row[2 + (a == 0 ? oa + 2 * ob : ob + 2 * oa)] * FV;
	return faceMean2(face2d(e, n, a, 2 * I - oa * n, 2 * t - ob * n), face2d(e, n, a, 2 * I - oa * n, 2 * t - ob * n + 1));
}

static __global__ __launch_bounds__(256) void k_facexfer2d(int n, int Pd, const int32_t *__restrict__ map, const double *__restrict__ hsrc,
                                                           const double *__restrict__ src, double *__restrict__ dst)
{
	const int    h = n / 2, nn = n * n;
	const size_t total = (size_t) Pd * n * h, FV = 2 * (size_t) nn + 2 * n;
	for (size_t idx = (size_t) blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t) gridDim.x * blockDim.x) {
		const int      pd = (int) (idx / ((size_t) n * h)), q = (int) (idx % ((size_t) n * h));
		const int      y = q / h, x = 2 * (q % h);
		const int32_t *row = map + (size_t) pd * RG_ROW;
		const int      kind = row[0], o = row[1];
		double        *dp = dst + (size_t) pd * FV;
		// copy, refine: the one source patch and its spacings (a coarsened patch finds its children in coarsenFace2d and uses neither)
		const double  *e = src + (size_t) row[2] * FV, *hs = hsrc + (size_t) row[2] * 3;
		// F_a(i; t) of the destination patch
		auto value = [&](int a, int i, int t) {
			if (kind == RG_COPY) return face2d(e, n, a, i, t);
			if (kind == RG_COARSEN) return coarsenFace2d(src, FV, row, n, a, i, t);
			return refineFace2d(e, n, hs, o, a, i, t);
		};
		*reinterpret_cast<double2 *>(dp + x + n * y)      = double2{value(0, x, y), value(0, x + 1, y)};
		*reinterpret_cast<double2 *>(dp + nn + x + n * y) = double2{value(1, y, x), value(1, y, x + 1)};
		if (x + 2 == n) dp[2 * nn + y] = value(0, n, y);
		if (y == n - 1) *reinterpret_cast<double2 *>(dp + 2 * nn + n + x) = double2{value(1, n, x), value(1, n, x + 1)};
	}
}
} // namespace te
