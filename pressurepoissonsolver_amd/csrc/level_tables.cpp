// The tables of one multigrid level, computed on the host (see level_tables.hpp). Plain C++: the layout facts it shares with
// the kernels come from table_layout.hpp.
#include "level_tables.hpp"
#include "capi_common.hpp"
#include "table_layout.hpp"
#include <algorithm>
#include <array>
#include <cmath>
#include <map>
#include <tuple>

using namespace te;

namespace tei
{
namespace
{
using PeerItems = std::vector<std::pair<int, int64_t>>; // (peer, doubles), sorted by peer

// DftPatchSolver.h:237-289 (row-major: y_i = sum_j M[i*n+j] x_j); type 0..5 = DCT-II, -III, -IV, DST-II, -III, -IV
void transformMatrix(int type, int n, double *m)
{
	static const double oi[6] = {0.0, 0.5, 0.5, 1.0, 0.5, 0.5}, oj[6] = {0.5, 0.0, 0.5, 0.5, 1.0, 0.5};
	for (int i = 0; i < n; i++) {
		for (int j = 0; j < n; j++) {
			const double x = M_PI / n * ((i + oi[type]) * (j + oj[type]));
			m[i * n + j]   = type < 3 ? cos(x) : sin(x);
		}
		if (type == 1) m[i * n] = 0.5;                          // (the constant term)
		if (type == 4) m[i * n + n - 1] = (i & 1) ? -0.5 : 0.5; // (the alternating term)
	}
}

// one exchange from its send-side and receive-side (peer, count) lists, each sorted by peer (counts > 0)
ExPlan mergePlan(const PeerItems &sends, const PeerItems &recvs)
{
	std::map<int, std::array<int64_t, 4>> m; // peer -> send_off, send_cnt, recv_off, recv_cnt
	auto ranges = [&m](const PeerItems &items, int at) {
		int64_t pos = 0;
		for (auto &it : items) {
			auto &e = m[it.first];
			if (e[at + 1] == 0) e[at] = pos; // (the peer's first item: its range starts here)
			e[at + 1] += it.second;
			pos += it.second;
		}
	};
	ranges(sends, 0);
	ranges(recvs, 2);
	ExPlan pl;
	for (auto &kv : m) {
		pl.peers.push_back(kv.first);
		pl.send_off.push_back(kv.second[0]);
		pl.send_cnt.push_back(kv.second[1]);
		pl.recv_off.push_back(kv.second[2]);
		pl.recv_cnt.push_back(kv.second[3]);
	}
	return pl;
}

// both ends of every axis of a patch-solve plan have the same boundary kind (key: bit s = side s is a Neumann boundary)
bool pureAxes(int key, int D)
{
	bool ok = true;
	for (int a = 0; a < D; a++) ok &= (((key >> (2 * a)) & 1) == ((key >> (2 * a + 1)) & 1));
	return ok;
}

// a global fact (all ranks and every partition take the same arithmetic path): the level is uniformly refined everywhere --
// no coarse/fine face, every patch an orthant child
bool uniformlyRefined(const Level &lv)
{
	const int NS = 2 * lv.dim;
	for (int gp = 0; gp < lv.P_global; gp++) {
		if (lv.g_orth_on_parent[gp] < 0) return false;
		for (int s = 0; s < NS; s++)
			if (lv.g_nbr_kind[(size_t) gp * NS + s] > NBR_NORMAL) return false;
	}
	return true;
}

// One table of `size` doubles per distinct (plan, spacings) among the patches whose plan is in `use`, numbered as they are first
// met: fill(table, plan, 1/hx^2, 1/hy^2, 1/hz^2) writes a new one; T.psitab[p] = the patch's table in T.psinv
template <class Fill> void tablesBySpacing(LevelTables &T, const std::vector<char> &use, size_t size, Fill fill)
{
	std::map<std::tuple<int, double, double, double>, int> which;
	T.psitab.assign(std::max(T.P, 1), 0);
	for (int p = 0; p < T.P; p++) {
		const int k = T.plan[p];
		if (!use[k]) continue;
		const double *r   = &T.rh2[(size_t) p * 3]; // (2D: r[2] = 0 on every patch)
		const auto    key = std::make_tuple(k, r[0], r[1], r[2]);
		auto          it  = which.find(key);
		if (it == which.end()) {
			it = which.emplace(key, (int) which.size()).first;
			T.psinv.resize(T.psinv.size() + size);
			fill(&T.psinv[(size_t) it->second * size], k, r[0], r[1], r[2]);
		}
		T.psitab[p] = it->second;
	}
	if (T.psinv.empty()) T.psinv.resize(1, 0.0);
}

// [patches whose plan is in `pure` | the others]; returns how many the first part has
int pureFirst(const LevelTables &T, const std::vector<char> &pure, std::vector<int32_t> &lst)
{
	std::vector<int32_t> mixed;
	for (int p = 0; p < T.P; p++) (pure[T.plan[p]] ? lst : mixed).push_back(p);
	const int n_pure = (int) lst.size();
	lst.insert(lst.end(), mixed.begin(), mixed.end());
	return n_pure;
}

// ---- remote same-level faces: canonical order = (peer, receiving patch (global), receiving side),
// which both ends can compute from the global tables
// A receiving (patch, side, q) gets ONE ghost slot holding the sender's facing layer: the ghost values
// themselves on a same-level face, raw neighbour cells for k_cf_ghost on a coarse/fine face (q = which
// of the finer neighbours; the coarse side of a coarse/fine face receives one slot per fine neighbour).
struct RFace {
	int peer, key_patch, key_side, key_q, p, s, nb;
	bool operator<(const RFace &o) const
	{
		return std::tie(peer, key_patch, key_side, key_q) < std::tie(o.peer, o.key_patch, o.key_side, o.key_q);
	}
};

// the face exchange: T.fx, nremote, send_faces, f6off. Returns the received faces in slot order.
std::vector<RFace> exchangePlan(const Level &lv, int me, LevelTables &T)
{
	const int          D = lv.dim, P = lv.P, NS = 2 * D, NQ = 1 << (D - 1);
	std::vector<RFace> recvs, sends;
	for (int p = 0; p < P; p++) {
		const int gp = lv.l2g[p];
		for (int s = 0; s < NS; s++) {
			const size_t gf   = (size_t) gp * NS + s;
			const int    kind = lv.g_nbr_kind[gf];
			if (kind == NBR_NONE) continue;
			for (int q = 0; q < NQ; q++) {
				const int nb = lv.g_nbr[gf * 4 + q];
				if (nb < 0 || lv.g_rank[nb] == me) continue;
				recvs.push_back({lv.g_rank[nb], gp, s, q, p, s, nb});
				// what the neighbour files my layer under: its own (patch, side) and, when it is the coarse
				// side, my position among its fine neighbours = my quadrant on its face
				const int their_q = (kind == NBR_COARSE) ? lv.g_nbr_orth[gf] : 0;
				sends.push_back({lv.g_rank[nb], nb, s ^ 1, their_q, p, s, nb});
			}
		}
	}
	std::sort(recvs.begin(), recvs.end());
	std::sort(sends.begin(), sends.end());
	PeerItems si, ri;
	for (auto &f : sends) {
		si.emplace_back(f.peer, (int64_t) T.nf);
		T.send_faces.push_back(f.p);
		T.send_faces.push_back(f.s);
	}
	for (auto &f : recvs) ri.emplace_back(f.peer, (int64_t) T.nf);
	T.fx      = mergePlan(si, ri);
	T.nremote = (int) recvs.size();
	if (D == 3 && T.nremote > 0) { // the place of every face layer in f6buf: sent layers first, in send order (see LevelHost::f6off)
		std::vector<int32_t> off((size_t) P * NS, -1);
		bool                 once = true;
		for (size_t i = 0; i < sends.size() && once; i++) {
			int32_t &o = off[(size_t) sends[i].p * NS + sends[i].s];
			once       = (o < 0);
			o          = (int32_t) i;
		}
		if (once) {
			int32_t next = (int32_t) sends.size();
			for (auto &o : off)
				if (o < 0) o = next++;
			T.f6off = std::move(off);
		}
	}
	return recvs;
}

// the stencil tables, the ghost slot numbering, the interior / boundary order and the patch geometry. Returns the boundary key
// of every patch-solve plan (T.plan[p] indexes it).
std::vector<int> stencilTables(const Level &lv, int me, int neumann_sides, const std::vector<RFace> &recvs, LevelTables &T)
{
	const int D = lv.dim, n = lv.n, P = lv.P, NS = 2 * D, NQ = 1 << (D - 1);
	std::map<std::tuple<int, int, int>, int> remote_slot; // (p, s, q) -> ghost slot
	for (int i = 0; i < T.nremote; i++) remote_slot[std::make_tuple(recvs[i].p, recvs[i].s, recvs[i].key_q)] = i;
	std::vector<int32_t> &fk = T.face_kind, &fs = T.face_src, &cfd = T.cf_desc;
	fk.assign(P * NS, 0);
	fs.assign(P * NS, -1);
	T.plan.assign(P, 0);
	T.face_kadj.assign(P * NS, 0.0);
	T.rh2.assign(P * 3, 0.0);
	T.cellvol.assign(P, 0.0);
	T.patch_vol.assign(P, 0.0);
	T.geom_starts.assign((size_t) P * 3, 0.0);
	T.geom_h.assign((size_t) P * 3, 1.0);
	T.node_ids.assign(P, 0);
	std::map<int, int> plan_of_key;
	std::vector<int>   keys;
	std::vector<int32_t> bnd;
	T.nslots = T.nremote;
	for (int p = 0; p < P; p++) {
		const int gp  = lv.l2g[p];
		int       key = 0;
		double    cv = 1.0, pv = 1.0; // Domain.h:270-272 (patch_sum *= spacings[i]), :242-245
		T.node_ids[p] = lv.g_id[gp];
		for (int a = 0; a < D; a++) {
			double h         = lv.g_lengths[(size_t) gp * D + a] / n;
			T.rh2[p * 3 + a] = 1.0 / (h * h);
			cv *= h;
			pv *= h * n;
			T.geom_starts[(size_t) p * 3 + a] = lv.g_starts[(size_t) gp * D + a];
			T.geom_h[(size_t) p * 3 + a]      = lv.g_lengths[(size_t) gp * D + a] / n;
		}
		T.cellvol[p]   = cv;
		T.patch_vol[p] = pv;
		bool ghost     = false;
		for (int s = 0; s < NS; s++) {
			const size_t gf   = (size_t) gp * NS + s;
			const int    kind = lv.g_nbr_kind[gf];
			if (kind == NBR_NONE) {
				const bool neumann      = (neumann_sides >> s) & 1; // one kind per side of the DOMAIN
				fk[p * NS + s]          = neumann ? FACE_NEUMANN : FACE_DIRICHLET;
				T.face_kadj[p * NS + s] = neumann ? -1.0 : 1.0;
				if (neumann) key |= 1 << s;
			} else if (kind == NBR_NORMAL) {
				const int nb = lv.g_nbr[gf * 4];
				if (lv.g_rank[nb] == me) {
					fk[p * NS + s] = FACE_LOCAL;
					fs[p * NS + s] = lv.g_local[nb];
				} else { // the neighbour's face cells arrive in a ghost slot; diagonal unchanged
					fk[p * NS + s] = FACE_GHOST;
					fs[p * NS + s] = remote_slot.at(std::make_tuple(p, s, 0));
				}
			} else {
				fk[p * NS + s]          = FACE_GHOST;
				fs[p * NS + s]          = T.nslots;
				T.face_kadj[p * NS + s] = (kind == NBR_COARSE) ? (D == 3 ? -5.0 / 6.0 : -2.0 / 3.0) : 1.0 / 3.0;
				cfd.push_back(p);
				cfd.push_back(s);
				cfd.push_back(kind);
				cfd.push_back(lv.g_nbr_orth[gf]);
				for (int q = 0; q < 4; q++) { // local patch index, or -(slot+2) of the raw layer received for it
					int nb = (q < NQ) ? lv.g_nbr[gf * 4 + q] : -1;
					if (nb >= 0 && lv.g_rank[nb] != me)
						cfd.push_back(-(remote_slot.at(std::make_tuple(p, s, q)) + 2));
					else
						cfd.push_back(nb >= 0 ? lv.g_local[nb] : -1);
				}
				T.cf_slots.push_back(T.nslots);
				T.nslots++;
			}
			ghost |= (fk[p * NS + s] == FACE_GHOST);
		}
		(ghost ? bnd : T.order).push_back(p); // interior patches (no ghost-slot face) first, then boundary patches
		auto it = plan_of_key.find(key);
		if (it == plan_of_key.end()) {
			it = plan_of_key.emplace(key, (int) keys.size()).first;
			keys.push_back(key);
		}
		T.plan[p] = it->second;
	}
	T.ncf   = (int) T.cf_slots.size();
	T.n_int = (int) T.order.size();
	T.n_bnd = (int) bnd.size();
	T.order.insert(T.order.end(), bnd.begin(), bnd.end());
	T.face_kind_patch = fk; // the PATCH operator: every neighbour face closed as homogeneous Dirichlet
	for (auto &k : T.face_kind_patch)
		if (k >= FACE_LOCAL) k = FACE_DIRICHLET;
	return keys;
}

// patch-solve plans (FftwPatchSolver.h:93-172: transform kinds per axis, eigenvalues): T.mats, lam, zero_mode
void planTransforms(const std::vector<int> &keys, int D, int n, LevelTables &T)
{
	const int np = (int) keys.size(), NS = 2 * D;
	T.mats.assign((size_t) np * 2 * D * n * n, 0.0);
	T.lam.assign((size_t) np * D * n, 0.0);
	T.zero_mode.assign(np, 0);
	for (int k = 0; k < np; k++) {
		const int key  = keys[k];
		T.zero_mode[k] = (key == (1 << NS) - 1);
		for (int a = 0; a < D; a++) {
			// boundary kinds of the axis' two ends (bit 0: lower end Neumann, bit 1: upper end): forward and inverse transform, and
			// the eigenvalues 4 sin^2((i + shift) pi / 2n)
			static const int    fwd[4] = {3, 2, 5, 0}, inv[4] = {4, 2, 5, 1};
			static const double shift[4] = {1.0, 0.5, 0.5, 0.0};
			const int           ends = (key >> (2 * a)) & 3;
			transformMatrix(fwd[ends], n, &T.mats[((size_t) k * 2 * D + a) * n * n]);
			transformMatrix(inv[ends], n, &T.mats[((size_t) k * 2 * D + D + a) * n * n]);
			for (int i = 0; i < n; i++) {
				const double s = sin((i + shift[ends]) * M_PI / (2 * n));
				T.lam[((size_t) k * D + a) * n + i] = 4 * s * s;
			}
		}
	}
}

// 3D, 32^3 patches: the three-pass kernels' matrices in lane order, k_ps_sym's fragments and reciprocal eigenvalue sums, and the
// per-patch choice between k_ps_sym and k_ps_fused
void solveTables32(const std::vector<int> &keys, LevelTables &T)
{
	const int                  np = (int) keys.size(), n = 32;
	const std::vector<double> &mats = T.mats, &lam = T.lam;
	T.matfrag.resize((size_t) np * 6 * 1024); // (table_layout.hpp matFragSource)
	for (int k = 0; k < np; k++)
		for (int m = 0; m < 6; m++)
			for (int e = 0; e < 16; e++)
				for (int ln = 0; ln < 64; ln++)
					T.matfrag[((size_t) k * 6 + m) * 1024 + ((size_t) (e >> 1) * 64 + ln) * 2 + (e & 1)] = mats[((size_t) k * 6 + m) * 1024 + matFragSource(m, ln, e)];
	// k_ps_sym's tables: [plan][transform 6][parity 2][k-step 4][lane 64]
	std::vector<double> &fs = T.matsym;
	fs.assign((size_t) np * PSS_FRAG, 0.0);
	std::vector<char> pure(np);
	for (int k = 0; k < np; k++) {
		pure[k] = pureAxes(keys[k], 3);
		for (int a = 0; a < 3; a++) {
			if (((keys[k] >> (2 * a)) & 1) != ((keys[k] >> (2 * a + 1)) & 1)) continue;
			const double *F = &mats[((size_t) k * 6 + a) * n * n], *G = &mats[((size_t) k * 6 + 3 + a) * n * n];
			for (int p = 0; p < 2; p++)
				for (int q = 0; q < 4; q++)
					for (int ln = 0; ln < 64; ln++) {
						const int j = ln & 15, g = ln >> 4;
						// forward: y as B operand and z as A operand take k = n = 4q + g, x as A operand k = g + 4q
						// (y comes first in the kernel: slot 0 = y, 1 = x, 2 = z)
						// inverse: x as B operand (k = m = 4q + g), y and z as A operands with k = m = g + 4q
						const int nf = (a == 0) ? g + 4 * q : 4 * q + g, mi = (a == 0) ? 4 * q + g : g + 4 * q;
						const int sf = (a == 0) ? 1 : (a == 1 ? 0 : 2);
						fs[(size_t) k * PSS_FRAG + ((sf * 2 + p) * 4 + q) * 64 + ln]      = F[(2 * j + p) * n + nf];
						// (the y inverse is the last product of the solve: its fragments carry the scale (2/N)^3 = 2^-12 of
						// DftPatchSolver.h:214 -- a power of two: the same bits as a multiplication of the result)
						fs[(size_t) k * PSS_FRAG + (((3 + a) * 2 + p) * 4 + q) * 64 + ln] = G[j * n + 2 * mi + p] * (a == 1 ? 8.0 / (32.0 * 32.0 * 32.0) : 1.0);
					}
		}
	}
	T.sym_ok = std::all_of(pure.begin(), pure.end(), [](char c) { return c != 0; });
	// k_ps_sym's reciprocal eigenvalue sums, among the patches with pure axes
	tablesBySpacing(T, pure, PSS_INV, [&](double *tab, int k, double rx, double ry, double rz) {
		const double *lx = &lam[((size_t) k * 3 + 0) * n], *ly = &lam[((size_t) k * 3 + 1) * n], *lz = &lam[((size_t) k * 3 + 2) * n];
		for (int half = 0; half < 2; half++)
			for (int sl = 0; sl < 16; sl++)
				for (int pp = 0; pp < 2; pp++)
					for (int r = 0; r < 4; r++)
						for (int c = 0; c < 2; c++)
							for (int ln = 0; ln < 64; ln++) {
								const int    j = ln & 15, g = ln >> 4, kx = 2 * sl + half, ky = 2 * j + c, kz = 2 * (g + 4 * r) + pp;
								const double ex = lx[kx] * rx, ey = ly[ky] * ry, ez = lz[kz] * rz;
								const double d  = -((ex + ey) + ez); // (FftwPatchSolver.h:143-168: the eigenvalue of the patch operator)
								// zero mode of an all-Neumann patch: the coefficient is set to zero (FftwPatchSolver.h:197)
								tab[((((size_t) (half * 16 + sl) * 2 + pp) * 4 + r) * 2 + c) * 64 + ln] = (T.zero_mode[k] && kx == 0 && ky == 0 && kz == 0) ? 0.0 : 1.0 / d;
							}
	});
	if (!T.sym_ok) T.n_pure = pureFirst(T, pure, T.ps_list);
}

// 2D, 64^2 patches: k_patch_solve2d_sym's tables (see there): stage 0 / 1 forward x / y, 2 / 3 inverse x / y
void solveTables64(const std::vector<int> &keys, LevelTables &T)
{
	const int                  np = (int) keys.size(), n = 64;
	const std::vector<double> &mats = T.mats, &lam = T.lam;
	std::vector<double>        fs((size_t) np * PS2S_PLAN, 0.0);
	std::vector<char>          pure(np);
	for (int k = 0; k < np; k++) {
		pure[k] = pureAxes(keys[k], 2);
		if (!pure[k]) continue;
		const double *Fx = &mats[((size_t) k * 4 + 0) * n * n], *Fy = &mats[((size_t) k * 4 + 1) * n * n];
		const double *Gx = &mats[((size_t) k * 4 + 2) * n * n], *Gy = &mats[((size_t) k * 4 + 3) * n * n];
		// the symmetry the kernel rests on: F[k][63 - j] = (-1)^k F[k][j], G[63 - j][k] = (-1)^k G[j][k]
		for (int i = 0; i < n && pure[k]; i++)
			for (int jj = 0; jj < n / 2; jj++) {
				const double sg = (i & 1) ? -1.0 : 1.0;
				const double e  = 1e-12;
				if (fabs(Fx[i * n + n - 1 - jj] - sg * Fx[i * n + jj]) > e || fabs(Fy[i * n + n - 1 - jj] - sg * Fy[i * n + jj]) > e
				    || fabs(Gx[(n - 1 - jj) * n + i] - sg * Gx[jj * n + i]) > e || fabs(Gy[(n - 1 - jj) * n + i] - sg * Gy[jj * n + i]) > e)
					pure[k] = 0;
			}
		if (!pure[k]) continue;
		double *S = &fs[(size_t) k * PS2S_PLAN];
		for (int ks = 0; ks < 8; ks++)
			for (int t = 0; t < 4; t++)
				for (int ln = 0; ln < 64; ln++) {
					const int    j = ln & 15, gq = ln >> 4, kk = 4 * ks + gq;
					const size_t e = ((size_t) ks * 4 + t) * 64 + ln;
					const int    wv = t < 2 ? 2 * (16 * t + j) : 2 * (16 * (t - 2) + j) + 1; // the wave number behind position 16 t + j
					S[0 * PS2S_STAGE + e] = Fx[wv * n + kk];
					S[1 * PS2S_STAGE + e] = Fy[wv * n + kk];
					S[2 * PS2S_STAGE + e] = Gx[(16 * (t & 1) + j) * n + 2 * kk + (t >> 1)];
					S[3 * PS2S_STAGE + e] = Gy[(16 * (t & 1) + j) * n + 2 * kk + (t >> 1)];
				}
	}
	// the reciprocal eigenvalues (times the transforms' scale) in the kernel's parity-split positions: position c < 32 holds wave
	// number 2c, c >= 32 holds 2 (c - 32) + 1
	tablesBySpacing(T, pure, (size_t) n * n, [&](double *tab, int k, double rx, double ry, double) {
		const double *lx = &lam[((size_t) k * 2 + 0) * n], *ly = &lam[((size_t) k * 2 + 1) * n];
		const double  sc = 4.0 / ((double) n * n);
		for (int rp = 0; rp < n; rp++)
			for (int cp = 0; cp < n; cp++) {
				const int    ky = rp < 32 ? 2 * rp : 2 * (rp - 32) + 1, kx = cp < 32 ? 2 * cp : 2 * (cp - 32) + 1;
				const double d  = -(lx[kx] * rx + ly[ky] * ry);
				tab[(size_t) rp * n + cp] = (T.zero_mode[k] && kx == 0 && ky == 0) ? 0.0 : sc / d;
			}
	});
	std::vector<int32_t> lst;
	T.n_pure2 = pureFirst(T, pure, lst);
	if (T.n_pure2 > 0) T.mat2sym = std::move(fs);
	if (T.n_pure2 > 0 && T.n_pure2 < T.P) T.ps2_list = std::move(lst); // (all or none pure: no list)
}

void solvePlans(const std::vector<int> &keys, LevelTables &T)
{
	const int D = T.dim, n = T.n;
	planTransforms(keys, D, n, T);
	if (D == 3 && n == 32) solveTables32(keys, T);
	if (D == 2 && n <= 64) { // the transform matrices transposed (k_patch_solve2d_lds)
		T.matsT.resize(T.mats.size());
		for (size_t m = 0; m < T.mats.size() / ((size_t) n * n); m++)
			for (int i = 0; i < n; i++)
				for (int j = 0; j < n; j++) T.matsT[m * n * n + (size_t) j * n + i] = T.mats[m * n * n + (size_t) i * n + j];
	}
	if (D == 2 && n == 64 && T.P > 0) solveTables64(keys, T);
}

// a restricted block (or, on the way down, an orthant of a coarse patch) that travels between ranks: canonical order on both
// ends = (peer, parent patch (global), orthant). o < 0: a patch that copies through (a whole patch, filed as orthant 0)
struct Blk {
	int     peer, gpar, o, patch;
	int64_t size;
	bool    operator<(const Blk &b) const { return std::make_tuple(peer, gpar, std::max(o, 0)) < std::make_tuple(b.peer, b.gpar, std::max(b.o, 0)); }
};

// lays sorted blocks out back to back from `pos` on: their (patch, orthant or -1) descriptors, offsets and (peer, size) items;
// returns the end
int64_t layOut(const std::vector<Blk> &blks, int64_t pos, std::vector<int32_t> &desc, std::vector<int64_t> &off, PeerItems &items)
{
	for (auto &b : blks) {
		desc.push_back(b.patch);
		desc.push_back(b.o);
		off.push_back(pos);
		items.emplace_back(b.peer, b.size);
		pos += b.size;
	}
	return pos;
}

// the same blocks with face-vector sizes (LevelTables::up_foff / down_foff): offsets from `pos` on and (peer, size) items; returns the end
int64_t layOutFaces(const std::vector<Blk> &blks, int64_t pos, int D, int n, std::vector<int64_t> &off, PeerItems &items)
{
	for (auto &b : blks) {
		const int64_t size = faceDoubles(D, b.o < 0 ? n : n / 2);
		off.push_back(pos);
		items.emplace_back(b.peer, size);
		pos += size;
	}
	return pos;
}

// restriction towards a level that lives on every rank: the same range [0, up_total) of the send buffer to every other rank (if this
// rank has patches here at all), and from every rank that has patches here its blocks (`downs`)
ExPlan replicatedUpPlan(const Hierarchy &H, const PeerItems &downs, int64_t up_total)
{
	const ExPlan pl = mergePlan({}, downs);
	if (up_total <= 0) return pl;
	ExPlan full;
	size_t k = 0;
	for (int r = 0; r < H.nranks; r++) {
		if (r == H.rank) continue;
		while (k < pl.peers.size() && pl.peers[k] < r) k++;
		const bool have = k < pl.peers.size() && pl.peers[k] == r;
		full.peers.push_back(r);
		full.send_off.push_back(0);
		full.send_cnt.push_back(up_total);
		full.recv_off.push_back(have ? pl.recv_off[k] : 0);
		full.recv_cnt.push_back(have ? pl.recv_cnt[k] : 0);
	}
	return full;
}

// The coarser level cv lives on every rank and lv does not: every local patch's restricted block goes to every other rank, and
// nothing comes back up. `downs`: the blocks this rank receives. Also: what that placement allows in 3D (post_exchange_free with
// slot_parent / slot_orth, and the in-place exchange tx_direct).
void replicatedPlans(const Hierarchy &H, const Level &lv, const Level &cv, const std::vector<RFace> &recvs, const PeerItems &downs,
                     LevelTables &T)
{
	const int me = H.rank;
	// restrict: the same range of upbuf to every other rank, and from every rank that has patches here its blocks; prolong: nothing
	T.tx_up = replicatedUpPlan(H, downs, T.up_total);
	if (lv.dim != 3) return;
	T.post_exchange_free = uniformlyRefined(lv);
	if (T.post_exchange_free && T.nremote > 0) {
		T.slot_parent.resize(T.nremote);
		T.slot_orth.resize(T.nremote);
		for (int i = 0; i < T.nremote; i++) {
			T.slot_parent[i] = cv.g_local[lv.g_parent[recvs[i].nb]];
			T.slot_orth[i]   = lv.g_orth_on_parent[recvs[i].nb];
		}
	}
	// in-place exchange of the restricted blocks: who fills which coarse patches
	std::vector<int> owner(cv.P_global, -1), lo(H.nranks, cv.P_global), hi(H.nranks, -1), cnt(H.nranks, 0);
	bool             direct = true;
	for (int gf = 0; gf < lv.P_global && direct; gf++) {
		int &o = owner[lv.g_parent[gf]];
		if (o >= 0 && o != lv.g_rank[gf]) direct = false;
		o = lv.g_rank[gf];
	}
	for (int pc = 0; pc < cv.P_global && direct; pc++) {
		const int r = owner[pc], lc = cv.g_local[pc];
		if (r < 0) {
			direct = false;
			break;
		}
		lo[r] = std::min(lo[r], lc), hi[r] = std::max(hi[r], lc), cnt[r]++;
	}
	for (int r = 0; r < H.nranks && direct; r++) direct = (cnt[r] == 0 || cnt[r] == hi[r] - lo[r] + 1);
	if (!direct) return;
	for (int r = 0; r < H.nranks; r++) {
		if (r == me || (cnt[r] == 0 && cnt[me] == 0)) continue;
		T.tx_direct.peers.push_back(r);
		T.tx_direct.send_off.push_back(cnt[me] ? (int64_t) lo[me] * (int64_t) T.nc : 0);
		T.tx_direct.send_cnt.push_back((int64_t) cnt[me] * (int64_t) T.nc);
		T.tx_direct.recv_off.push_back(cnt[r] ? (int64_t) lo[r] * (int64_t) T.nc : 0);
		T.tx_direct.recv_cnt.push_back((int64_t) cnt[r] * (int64_t) T.nc);
	}
	T.repl_direct = true;
}

// transfers to the coarser level cv. A child (or a copy-through patch) whose parent lives on another rank ships its restricted
// block there; the parent's rank ships octant blocks back for prolongation. Reads the stencil tables of T (face_kind, face_src,
// ncf, nslots, lds2d).
int transferTables(const Hierarchy &H, const Level &lv, const Level &cv, const LevelBuildOpts &opt, const std::vector<RFace> &recvs,
                   LevelTables &T)
{
	const int D = lv.dim, n = lv.n, P = lv.P, NCH = 1 << D, me = H.rank;
	std::vector<int32_t> &parent = T.parent, &orth = T.orth, &child = T.child, &copy = T.copy;
	parent.assign(P, 0);
	orth.assign(P, 0);
	child.assign((size_t) cv.P * NCH, -1);
	copy.assign(cv.P, 0);
	auto blk = [&](int peer, int gpar, int o, int patch) { return Blk{peer, gpar, o, patch, (int64_t) (o < 0 ? T.nc : T.nc / NCH)}; };
	std::vector<Blk> up, down;
	T.repl_up = cv.replicated && !lv.replicated;
	for (int p = 0; p < P; p++) {
		const int gp = lv.l2g[p], gpar = lv.g_parent[gp];
		orth[p]      = lv.g_orth_on_parent[gp];
		if (cv.g_rank[gpar] == me) {
			const int pc = cv.g_local[gpar];
			parent[p]    = pc;
			if (orth[p] < 0) copy[pc] = 1;
			child[(size_t) pc * NCH + std::max(orth[p], 0)] = p;
		} else {
			up.push_back(blk(cv.g_rank[gpar], gpar, orth[p], p));
		}
	}
	for (int gf = 0; gf < lv.P_global; gf++) {
		const int gpar = lv.g_parent[gf];
		if (cv.g_rank[gpar] != me || lv.g_rank[gf] == me) continue;
		const int o = lv.g_orth_on_parent[gf];
		down.push_back(blk(lv.g_rank[gf], gpar, o, cv.g_local[gpar]));
		if (o < 0) copy[cv.g_local[gpar]] = 1;
	}
	std::sort(up.begin(), up.end());
	std::sort(down.begin(), down.end());
	PeerItems ups, downs, none, fups, fdowns, fnone;
	T.up_total  = layOut(up, 0, T.up_desc, T.up_off, ups);
	T.up_ftotal = layOutFaces(up, 0, D, n, T.up_foff, fups);
	for (size_t i = 0; i < up.size(); i++) parent[up[i].patch] = -((int) i + 2); // prolong reads block i of upbuf
	if (T.repl_up) { // (up is empty: every parent is local) one block per local patch, in the order the receivers expect: (parent, orthant)
		std::vector<Blk> bc;
		for (int p = 0; p < P; p++) bc.push_back(blk(0, lv.g_parent[lv.l2g[p]], orth[p], p));
		std::sort(bc.begin(), bc.end());
		// up_desc (fine patch, orthant): k_restrict_pack restricts it into its block; bc_desc (coarse patch, orthant or -1):
		// k_prolong_pack copies the finished octant out
		T.up_total  = layOut(bc, T.up_total, T.up_desc, T.up_off, none);
		T.up_ftotal = layOutFaces(bc, T.up_ftotal, D, n, T.up_foff, fnone);
		for (auto &b : bc) {
			T.bc_desc.push_back(parent[b.patch]);
			T.bc_desc.push_back(b.o);
		}
	}
	T.down_total  = layOut(down, 0, T.down_desc, T.down_off, downs);
	T.down_ftotal = layOutFaces(down, 0, D, n, T.down_foff, fdowns);
	for (size_t i = 0; i < down.size(); i++) // restrict reads block i of downbuf
		child[(size_t) down[i].patch * NCH + std::max(down[i].o, 0)] = -((int) i + 2);
	for (int pc = 0; pc < cv.P; pc++) {
		if (copy[pc]) continue;
		for (int o = 0; o < NCH; o++)
			if (child[(size_t) pc * NCH + o] == -1) return te::fail(TE_EINVAL, "te_gmg_create: coarse patch with a missing child");
	}
	T.Pc     = cv.P;
	T.n_up   = (int) (T.up_desc.size() / 2);
	T.n_down = (int) down.size();
	// (repl_up: the blocks in `down` are received for the restriction only; every parent is local)
	const bool parents_local = up.empty() && (down.empty() || T.repl_up);
	const bool all_children  = std::all_of(orth.begin(), orth.end(), [](int32_t o) { return o >= 0; });
	T.has_copy               = !all_children;
	T.prolong_fusable        = (D == 3 && T.ncf == 0 && parents_local && all_children);
	T.prolong_fusable_cf     = (D == 3 && parents_local && !opt.no_cfp);
	if (D == 2 && T.lds2d && parents_local) { // (no transfers, or a coarse level on every rank: its blocks travel behind the kernels)
		T.fuse2d          = true;
		// (faces on other ranks are fine: their values of u + P e arrive in ghost slots, packProlongFaces2d)
		T.prolong_fusable = ((opt.no_mr_fuse_2d ? T.nslots == 0 : T.ncf == 0) && all_children);
	}
	if (D == 2 && T.lds2d) T.fuse2_ok = uniformlyRefined(lv); // the 3D fusions in 2D (kernels2d.hpp): a global fact, as in 3D
	if (T.repl_up) {
		replicatedPlans(H, lv, cv, recvs, downs, T);
		T.tx_fup = replicatedUpPlan(H, fdowns, T.up_ftotal);
	} else {
		T.tx_up   = mergePlan(ups, downs); // restrict: send child blocks, receive into downbuf
		T.tx_down = mergePlan(downs, ups); // prolong: send octants, receive into upbuf
		T.tx_fup  = mergePlan(fups, fdowns); // the restriction of a face vector: the same blocks with face-vector sizes
	}
	if (T.prolong_fusable && D == 3) { // ProlongSrc::cbase: coarseOctant() of every patch and of its six neighbours, precomputed
		const int64_t nn = (int64_t) n * n, nnn = nn * n, hh = n / 2;
		auto          base = [&](int p) {
            const int o = orth[p];
            return (int64_t) parent[p] * nnn + ((o & 1) ? hh : 0) + n * ((o & 2) ? hh : 0) + nn * ((o & 4) ? hh : 0);
		};
		T.cbase.assign((size_t) std::max(P, 1) * 7, -1);
		for (int p = 0; p < P; p++) {
			T.cbase[(size_t) p * 7] = base(p);
			for (int s = 0; s < 6; s++)
				if (T.face_kind[(size_t) p * 6 + s] == FACE_LOCAL) T.cbase[(size_t) p * 7 + 1 + s] = base(T.face_src[(size_t) p * 6 + s]);
		}
	}
	return TE_OK;
}

// LevelTables::brestrict. A child's physical side s is a physical side s of its parent, so the map follows from parent, orth and
// the two levels' physical-face numbers.
int boundaryRestrictTable(const Level &lv, const Level &cv, LevelTables &T)
{
	const int            D = lv.dim, NS = 2 * D, NQ = 1 << (D - 1);
	std::vector<int32_t> cb;
	const int            ncb = te::bfaceIndex(cv, cb);
	T.brestrict.assign((size_t) ncb * 5, -1);
	for (int p = 0; p < lv.P; p++) {
		const int pc = T.parent[p], o = T.orth[p];
		for (int s = 0; s < NS; s++) {
			const int fb = T.bface[(size_t) p * NS + s];
			if (fb < 0) continue;
			const int c = cb[(size_t) pc * NS + s];
			if (c < 0) return te::fail(TE_EINVAL, "te_gmg_create: a physical face whose parent has a neighbour there");
			int32_t *row = &T.brestrict[(size_t) c * 5];
			if (o < 0) {
				row[0] = 1, row[1] = fb;
				continue;
			}
			int q = 0, k = 0;
			for (int a = 0; a < D; a++)
				if (a != (s >> 1)) q |= ((o >> a) & 1) << k++;
			row[0] = 0, row[1 + q] = fb;
		}
	}
	for (int c = 0; c < ncb; c++) {
		const int32_t *row = &T.brestrict[(size_t) c * 5];
		bool           ok  = row[0] == 1 ? row[1] >= 0 : row[0] == 0;
		for (int q = 0; ok && row[0] == 0 && q < NQ; q++) ok = row[1 + q] >= 0;
		if (!ok) return te::fail(TE_EINVAL, "te_gmg_create: a coarse physical face that its children do not cover");
	}
	return TE_OK;
}
} // namespace

int computeLevelTables(const Hierarchy &H, int li, const LevelBuildOpts &opt, LevelTables &T)
{
	const Level &lv = H.levels[li];
	const int    n = lv.n, D = lv.dim;
	T            = LevelTables();
	T.dim        = D;
	T.n          = n;
	T.P          = lv.P;
	T.P_global   = lv.P_global;
	T.nif        = lv.num_ifaces;
	T.if_own     = lv.iface_own;
	T.if_start   = lv.iface_start;
	T.if_contrib = lv.iface_contrib;
	T.nbf        = te::bfaceIndex(lv, T.bface);
	T.replicated = lv.replicated;
	T.gathered   = lv.replicated || (H.nranks > 1 && std::all_of(lv.g_rank.begin(), lv.g_rank.end(), [&](int32_t r) { return r == lv.g_rank[0]; }));
	T.nc         = (D == 3) ? (size_t) n * n * n : (size_t) n * n;
	T.nf         = (D == 3) ? (size_t) n * n : (size_t) n;
	const bool coarser = li + 1 < (int) H.levels.size();

	const std::vector<RFace> recvs = exchangePlan(lv, H.rank, T);
	const std::vector<int>   keys  = stencilTables(lv, H.rank, H.neumann_sides, recvs, T);
	T.lds2d = (D == 2 && n <= 64 && n % 2 == 0 && !opt.simple_2d);
	// see LevelHost::fuse2_ok: a global fact only. (Refined levels qualify: patches that copy through and
	// coarse/fine faces -- whose ghost slots carry the interpolated value -- are handled by both kernels.)
	T.fuse2_ok = (D == 3 && coarser && lv.P_global >= 256); // (TE_NO_FUSE2 is looked at where the path is chosen)
	solvePlans(keys, T);
	T.coarser = coarser;
	if (!coarser) return TE_OK;
	if (int rc = transferTables(H, lv, H.levels[li + 1], opt, recvs, T)) return rc;
	return H.nranks == 1 ? boundaryRestrictTable(lv, H.levels[li + 1], T) : TE_OK; // (every parent is local)
}
} // namespace tei
