// Host-only check of pressurepoissonsolver_amd/csrc/level_tables.cpp (driven by tests/test_level_tables.py): builds the
// hierarchies of the committed meshes for every rank of 1, 2, 4 and 8-rank partitions in ONE process, computes every rank's level
// tables and verifies what the kernels and the exchanges take for granted -- all exact integer facts:
//   * what rank a sends to b in any exchange plan is what b expects from a, and the faces of the face exchange arrive in the ghost
//     slots the receiver filed them under (the canonical order both ends compute on their own);
//   * every index a kernel follows without checking is in range;
//   * order, ps_list and ps2_list are the permutations they are documented to be; parent / child / copy agree.
// usage: level_tables_check <directory of the mesh files>; exit status 0 and "OK <cases>" when everything holds.
#include "../pressurepoissonsolver_amd/csrc/capi_common.hpp"
#include "../pressurepoissonsolver_amd/csrc/level_tables.hpp"
#include "../pressurepoissonsolver_amd/csrc/table_layout.hpp"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>

using namespace te;
using namespace tei;

namespace te
{
int fail(int code, const std::string &msg) // (the library's own lives in capi_mesh.cpp)
{
	fprintf(stderr, "te::fail(%d): %s\n", code, msg.c_str());
	return code;
}
} // namespace te

static std::string g_case; // what is being checked, for the message
static int         g_failures = 0;
#define CHECK(cond, ...)                                             \
	do {                                                             \
		if (!(cond)) {                                               \
			fprintf(stderr, "FAILED [%s] %s: ", g_case.c_str(), #cond); \
			fprintf(stderr, __VA_ARGS__);                            \
			fprintf(stderr, "\n");                                   \
			if (++g_failures >= 20) exit(1);                         \
		}                                                            \
	} while (0)

// doubles rank `peer` is sent (send = true) or sends us in plan pl
static int64_t count(const ExPlan &pl, int peer, bool send)
{
	for (size_t i = 0; i < pl.peers.size(); i++)
		if (pl.peers[i] == peer) return (send ? pl.send_cnt : pl.recv_cnt)[i];
	return 0;
}

static bool isPermutation(const std::vector<int32_t> &v, int P)
{
	std::vector<int32_t> s(v);
	std::sort(s.begin(), s.end());
	for (int i = 0; i < (int) s.size(); i++)
		if (s[i] != i) return false;
	return (int) s.size() == P;
}

// every plan's axes have the same boundary kind at both ends, read off the stencil table
static bool pureAxes(const LevelTables &T, int p)
{
	for (int a = 0; a < T.dim; a++)
		if ((T.face_kind[(size_t) p * 2 * T.dim + 2 * a] == FACE_NEUMANN) != (T.face_kind[(size_t) p * 2 * T.dim + 2 * a + 1] == FACE_NEUMANN))
			return false;
	return true;
}

// the tables of one rank on one level, on their own
static void checkLocal(const Level &lv, const LevelTables &T)
{
	const int D = T.dim, P = T.P, NS = 2 * D, NCH = 1 << D;
	CHECK(P == lv.P && T.n_int + T.n_bnd == P, "P %d n_int %d n_bnd %d", P, T.n_int, T.n_bnd);
	CHECK(T.nslots == T.nremote + T.ncf && (int) T.cf_slots.size() == T.ncf, "nslots %d", T.nslots);
	std::vector<char> has_ghost(P, 0);
	for (int f = 0; f < P * NS; f++) {
		const int k = T.face_kind[f], src = T.face_src[f];
		if (k == FACE_LOCAL) CHECK(src >= 0 && src < P, "face %d: local neighbour %d of %d", f, src, P);
		if (k == FACE_GHOST) CHECK(src >= 0 && src < T.nslots, "face %d: ghost slot %d of %d", f, src, T.nslots);
		if (k == FACE_GHOST) has_ghost[f / NS] = 1;
	}
	std::set<int32_t> slots(T.cf_slots.begin(), T.cf_slots.end());
	CHECK((int) slots.size() == T.ncf, "cf_slots repeat a slot");
	for (int32_t s : T.cf_slots) CHECK(s >= T.nremote && s < T.nslots, "cf slot %d outside [%d, %d)", s, T.nremote, T.nslots);
	CHECK((int) T.cf_desc.size() == 8 * T.ncf, "cf_desc size");
	for (size_t i = 0; i < T.cf_desc.size(); i += 8) {
		CHECK(T.cf_desc[i] >= 0 && T.cf_desc[i] < P && T.cf_desc[i + 1] >= 0 && T.cf_desc[i + 1] < NS, "cf face %zu", i / 8);
		for (int q = 0; q < 4; q++) { // a local patch, -1 = none, or -(slot + 2)
			const int e = T.cf_desc[i + 4 + q];
			CHECK(e < P && (e >= -1 || -(e + 2) < T.nremote), "cf face %zu neighbour %d: %d", i / 8, q, e);
		}
	}
	CHECK(isPermutation(T.order, P), "order is no permutation");
	for (int i = 0; i < P && i < (int) T.order.size(); i++)
		CHECK(has_ghost[T.order[i]] == (i >= T.n_int), "order[%d] = %d is on the wrong side of n_int = %d", i, T.order[i], T.n_int);
	if (T.coarser) {
		CHECK((int) T.parent.size() == P && (int) T.child.size() == T.Pc * NCH && (int) T.copy.size() == T.Pc, "transfer table sizes");
		for (int p = 0; p < P; p++) {
			const int pc = T.parent[p], o = T.orth[p];
			CHECK(pc != -1 && pc < T.Pc && (pc >= 0 || -(pc + 2) < (int) T.up_desc.size() / 2), "parent[%d] = %d", p, pc);
			if (pc < 0) continue;
			CHECK(T.child[(size_t) pc * NCH + std::max(o, 0)] == p, "child[parent[%d]][%d] = %d", p, o, T.child[(size_t) pc * NCH + std::max(o, 0)]);
			if (o < 0) CHECK(T.copy[pc] == 1, "patch %d copies through, copy[%d] = %d", p, pc, T.copy[pc]);
		}
		for (int pc = 0; pc < T.Pc; pc++)
			for (int o = 0; o < NCH; o++) {
				const int c = T.child[(size_t) pc * NCH + o];
				CHECK(c < P && (c >= -1 || -(c + 2) < T.n_down) && (c != -1 || (T.copy[pc] && o > 0)), "child[%d][%d] = %d", pc, o, c);
			}
	}
	// patch-solve lists
	std::vector<char> pure(P);
	for (int p = 0; p < P; p++) pure[p] = pureAxes(T, p);
	const int  n_pure = (int) std::count(pure.begin(), pure.end(), 1);
	const auto pureFirst = [&](const std::vector<int32_t> &lst, int n_first, const char *name) {
		CHECK(isPermutation(lst, P) && n_first == n_pure, "%s: no permutation, or %d pure patches of %d", name, n_first, n_pure);
		for (int i = 0; i < (int) lst.size(); i++) CHECK(pure[lst[i]] == (i < n_first), "%s[%d] = %d", name, i, lst[i]);
	};
	if (D == 3 && T.n == 32) {
		CHECK(T.sym_ok == (n_pure == P) && T.ps_list.empty() == T.sym_ok, "sym_ok %d with %d pure of %d", (int) T.sym_ok, n_pure, P);
		if (!T.ps_list.empty()) pureFirst(T.ps_list, T.n_pure, "ps_list");
	}
	if (D == 2 && T.n == 64 && P > 0) {
		CHECK(T.n_pure2 == n_pure && T.ps2_list.empty() == (n_pure == 0 || n_pure == P), "n_pure2 %d, pure %d of %d", T.n_pure2, n_pure, P);
		if (!T.ps2_list.empty()) pureFirst(T.ps2_list, T.n_pure2, "ps2_list");
	}
	if (!T.psitab.empty()) {
		const size_t tab = (D == 3) ? (size_t) PSS_INV : (size_t) T.n * T.n, ntab = T.psinv.size() / tab;
		CHECK(T.psinv.size() == std::max<size_t>(ntab * tab, 1), "psinv holds %zu doubles", T.psinv.size());
		for (int p = 0; p < P; p++) CHECK(T.psitab[p] >= 0 && (size_t) T.psitab[p] < std::max<size_t>(ntab, 1), "psitab[%d] = %d", p, T.psitab[p]);
	}
}

// ghost slot -> the patch (global index) whose layer the receiver files there, and the receiving side; from the receiver's tables
static void slotSources(const Level &lv, const LevelTables &T, std::vector<int> &from, std::vector<int> &side)
{
	const int NS = 2 * T.dim;
	from.assign(T.nremote, -1);
	side.assign(T.nremote, -1);
	auto file = [&](int slot, int p, int s, int q) {
		CHECK(slot >= 0 && slot < T.nremote && from[slot] == -1, "ghost slot %d is filled twice (or does not exist)", slot);
		if (slot < 0 || slot >= T.nremote) return;
		from[slot] = lv.g_nbr[((size_t) lv.l2g[p] * NS + s) * 4 + q];
		side[slot] = s;
	};
	for (int f = 0; f < T.P * NS; f++)
		if (T.face_kind[f] == FACE_GHOST && T.face_src[f] < T.nremote) file(T.face_src[f], f / NS, f % NS, 0);
	for (size_t i = 0; i < T.cf_desc.size(); i += 8)
		for (int q = 0; q < 4; q++)
			if (T.cf_desc[i + 4 + q] <= -2) file(-(T.cf_desc[i + 4 + q] + 2), T.cf_desc[i], T.cf_desc[i + 1], q);
	for (int i = 0; i < T.nremote; i++) CHECK(from[i] >= 0, "ghost slot %d is never read", i);
}

// all ranks' tables of one level against each other
static void checkExchanges(const std::vector<Hierarchy> &H, const std::vector<LevelTables> &T, int li)
{
	const int    R        = (int) H.size();
	const char  *names[4] = {"fx", "tx_up", "tx_down", "tx_direct"};
	const ExPlan LevelTables::*plans[4] = {&LevelTables::fx, &LevelTables::tx_up, &LevelTables::tx_down, &LevelTables::tx_direct};
	for (int k = 0; k < 4; k++)
		for (int a = 0; a < R; a++) {
			const ExPlan &pl = T[a].*plans[k];
			if (R == 1) CHECK(pl.empty(), "%s is not empty on one rank", names[k]);
			CHECK(std::is_sorted(pl.peers.begin(), pl.peers.end()) && count(pl, a, true) == 0 && count(pl, a, false) == 0, "%s peers of rank %d", names[k], a);
			for (int b = 0; b < R; b++)
				CHECK(count(pl, b, true) == count(T[b].*plans[k], a, false), "%s: rank %d sends %lld to %d, which expects %lld", names[k], a,
				      (long long) count(pl, b, true), b, (long long) count(T[b].*plans[k], a, false));
		}
	if (R == 1) CHECK(T[0].nremote == 0, "nremote = %d on one rank", T[0].nremote);
	// the i-th face a sends to b is the face b files under its i-th receive slot from a
	std::vector<std::vector<int>> from(R), side(R);
	for (int b = 0; b < R; b++) slotSources(H[b].levels[li], T[b], from[b], side[b]);
	for (int a = 0; a < R; a++) {
		const ExPlan &pa = T[a].fx;
		const int64_t nf = (int64_t) T[a].nf;
		CHECK((int) T[a].send_faces.size() == 2 * T[a].nremote, "send_faces of rank %d", a);
		for (size_t k = 0; k < pa.peers.size(); k++) {
			const int     b  = pa.peers[k];
			const ExPlan &pb = T[b].fx;
			const size_t  kb = std::find(pb.peers.begin(), pb.peers.end(), a) - pb.peers.begin();
			if (kb == pb.peers.size() || pb.recv_cnt[kb] != pa.send_cnt[k]) continue; // (reported above)
			for (int64_t i = 0; i < pa.send_cnt[k] / nf; i++) {
				const int     p = T[a].send_faces[2 * (pa.send_off[k] / nf + i)], s = T[a].send_faces[2 * (pa.send_off[k] / nf + i) + 1];
				const int64_t slot = pb.recv_off[kb] / nf + i;
				CHECK(slot < T[b].nremote && from[b][slot] == H[a].levels[li].l2g[p] && side[b][slot] == (s ^ 1),
				      "face %lld from rank %d to %d: sent patch %d side %d, slot %lld holds patch %d for side %d", (long long) i, a, b,
				      H[a].levels[li].l2g[p], s, (long long) slot, slot < T[b].nremote ? from[b][slot] : -1, slot < T[b].nremote ? side[b][slot] : -1);
			}
		}
	}
}

static int runCase(const Tree &tree, int n, bool neumann, int nranks, const Placement &pl)
{
	std::vector<Hierarchy> H;
	for (int r = 0; r < nranks; r++) H.push_back(Hierarchy::build(tree, n, neumann, 0, 0.0, r, nranks, pl));
	for (int li = 0; li < (int) H[0].levels.size(); li++) {
		std::vector<LevelTables> T(nranks);
		const std::string        base = g_case;
		for (int r = 0; r < nranks; r++) {
			g_case = base + " level " + std::to_string(li) + " rank " + std::to_string(r);
			CHECK(computeLevelTables(H[r], li, LevelBuildOpts(), T[r]) == TE_OK, "computeLevelTables failed");
			checkLocal(H[r].levels[li], T[r]);
		}
		g_case = base + " level " + std::to_string(li);
		checkExchanges(H, T, li);
		g_case = base;
	}
	return 1;
}

int main(int argc, char **argv)
{
	if (argc != 2) return fprintf(stderr, "usage: %s <mesh directory>\n", argv[0]), 2;
	const struct {
		const char *file;
		int         dim, n_small, n_big;
	} meshes[] = {{"2refine.bin", 3, 8, 32}, {"multi_refine_8.bin", 3, 4, 32}, {"2d2ref.bin", 2, 8, 64}, {"2d_multi_refine_8.bin", 2, 8, 64}};
	// the small levels spread over the ranks, gathered on rank 0, and replicated on every rank
	const Placement placements[3] = {{0.0, -1, 0}, {16.0, -1, 0}, {16.0, -1, 1}};
	int             cases = 0;
	for (auto &m : meshes)
		for (int divides = 0; divides < 2; divides++) {
			Tree tree = Tree::read(std::string(argv[1]) + "/" + m.file, m.dim);
			for (int d = 0; d < divides; d++) tree.refineLeaves();
			for (int neumann = 0; neumann < 2; neumann++)
				for (int nranks : {1, 2, 4, 8})
					for (int ip = 0; ip < (nranks == 1 ? 1 : 3); ip++)
						for (int n : {m.n_small, m.n_big}) {
							if (n == m.n_big && (divides > 0 || nranks > 2 || ip == 1)) continue; // (the big tables: the patch-solve lists)
							g_case = std::string(m.file) + " divides " + std::to_string(divides) + " n " + std::to_string(n) + (neumann ? " neumann" : "")
							         + " ranks " + std::to_string(nranks) + " placement " + std::to_string(ip);
							cases += runCase(tree, n, neumann != 0, nranks, placements[ip]);
						}
		}
	if (g_failures) return fprintf(stderr, "%d checks failed\n", g_failures), 1;
	printf("OK %d cases\n", cases);
	return 0;
}
