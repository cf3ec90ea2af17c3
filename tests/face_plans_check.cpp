// Host-only check of the FACE-sized transfer plans of pressurepoissonsolver_amd/csrc/level_tables.cpp (driven by
// tests/test_face_plans_host.py): the layout the restriction of a face vector uses when children and parents live on different
// ranks (LevelTables::up_foff / down_foff / up_ftotal / down_ftotal / tx_fup). Builds the hierarchies of the committed meshes for
// every rank of 1, 2, 3, 4 and 8-rank partitions in ONE process, under the three placements of the small levels (spread, gathered
// on rank 0, replicated), and verifies -- all exact integer facts:
//   * every block (F(n/2) doubles for an orthant, F(n) for a patch that copies through, F(m) = D m^D + D m^(D-1)) lies inside its
//     buffer, no two blocks of a buffer overlap, and the blocks fill it;
//   * the block order is the cell plan's: a block goes to / comes from the same peer in tx_fup as in tx_up, in the same order;
//   * for every ordered pair (r, q) what r's face plan sends to q is what q's expects from r: the same count, and block for block
//     the same (parent, orthant) at the same place of the message;
//   * on the receiving rank every child of a local coarse patch has exactly one source -- the local fine patch or one received
//     block, each block used once (under repl_up: every rank's blocks cover each coarse patch's children exactly once);
//   * one rank: all face totals are zero and the plan is empty.
// usage: face_plans_check <directory of the mesh files>; exit status 0 and "OK <cases>" when everything holds.
#include "../pressurepoissonsolver_amd/csrc/capi_common.hpp"
#include "../pressurepoissonsolver_amd/csrc/level_tables.hpp"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <tuple>

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

static std::string g_case;
static int         g_failures = 0;
static long        g_blocks = 0, g_copy_blocks = 0, g_repl_levels = 0; // what the run actually saw (printed: a run over empty plans proves nothing)
#define CHECK(cond, ...)                                             \
	do {                                                             \
		if (!(cond)) {                                               \
			fprintf(stderr, "FAILED [%s] %s: ", g_case.c_str(), #cond); \
			fprintf(stderr, __VA_ARGS__);                            \
			fprintf(stderr, "\n");                                   \
			if (++g_failures >= 20) exit(1);                         \
		}                                                            \
	} while (0)

static int64_t F(int D, int64_t m) { return D == 3 ? 3 * m * m * m + 3 * m * m : 2 * m * m + 2 * m; }

// index of the peer whose range [off, off + cnt) of a plan holds `pos`, -1 if none; `several`: more than one does
static int rangeOf(const std::vector<int64_t> &off, const std::vector<int64_t> &cnt, int64_t pos, bool *several)
{
	int hit = -1;
	for (size_t k = 0; k < off.size(); k++)
		if (cnt[k] > 0 && pos >= off[k] && pos < off[k] + cnt[k]) {
			if (hit >= 0) *several = true;
			hit = (int) k;
		}
	return hit;
}

// one buffer's blocks: inside the total, disjoint, and filling it
static void checkBuffer(const char *name, int D, int n, const std::vector<int32_t> &desc, const std::vector<int64_t> &foff, int64_t total)
{
	CHECK(foff.size() * 2 == desc.size(), "%s: %zu offsets for %zu blocks", name, foff.size(), desc.size() / 2);
	if (foff.size() * 2 != desc.size()) return;
	std::vector<std::pair<int64_t, int64_t>> span; // (offset, size)
	int64_t                                  sum = 0;
	for (size_t i = 0; i < foff.size(); i++) {
		const int64_t size = F(D, desc[2 * i + 1] < 0 ? n : n / 2);
		CHECK(foff[i] >= 0 && foff[i] + size <= total, "%s block %zu: [%lld, +%lld) outside %lld", name, i, (long long) foff[i], (long long) size, (long long) total);
		span.emplace_back(foff[i], size);
		sum += size;
	}
	std::sort(span.begin(), span.end());
	for (size_t i = 0; i + 1 < span.size(); i++)
		CHECK(span[i].first + span[i].second <= span[i + 1].first, "%s: blocks at %lld and %lld overlap", name, (long long) span[i].first, (long long) span[i + 1].first);
	CHECK(sum == total, "%s: blocks hold %lld doubles, the total is %lld", name, (long long) sum, (long long) total);
}

struct Msg { // one block of a message: which child it is and where it sits relative to the message's start
	int     gpar, o;
	int64_t at;
	bool    operator==(const Msg &b) const { return std::tie(gpar, o, at) == std::tie(b.gpar, b.o, b.at); }
};

static void checkLevel(const std::vector<Hierarchy> &H, const std::vector<LevelTables> &T, int li)
{
	const int R = (int) H.size(), D = T[0].dim, n = T[0].n, NCH = 1 << D;
	for (int r = 0; r < R; r++) {
		const LevelTables &t = T[r];
		const std::string  who = "rank " + std::to_string(r);
		if (R == 1) CHECK(t.up_ftotal == 0 && t.down_ftotal == 0 && t.tx_fup.empty() && t.up_foff.empty() && t.down_foff.empty(), "one rank: face totals %lld / %lld", (long long) t.up_ftotal, (long long) t.down_ftotal);
		checkBuffer((who + " up").c_str(), D, n, t.up_desc, t.up_foff, t.up_ftotal);
		checkBuffer((who + " down").c_str(), D, n, t.down_desc, t.down_foff, t.down_ftotal);
		// the cell plan's order and peers
		const ExPlan &pc = t.tx_up, &pf = t.tx_fup;
		CHECK(pc.peers == pf.peers, "%s: tx_fup has other peers than tx_up", who.c_str());
		CHECK(std::is_sorted(pf.peers.begin(), pf.peers.end()) && std::find(pf.peers.begin(), pf.peers.end(), r) == pf.peers.end(), "%s: peers", who.c_str());
		if (pc.peers != pf.peers) continue;
		for (size_t k = 0; k < pf.peers.size(); k++) {
			CHECK(pf.send_off[k] >= 0 && pf.send_off[k] + pf.send_cnt[k] <= t.up_ftotal, "%s: send range %zu outside the buffer", who.c_str(), k);
			CHECK(pf.recv_off[k] >= 0 && pf.recv_off[k] + pf.recv_cnt[k] <= t.down_ftotal, "%s: recv range %zu outside the buffer", who.c_str(), k);
			CHECK((pf.send_cnt[k] > 0) == (pc.send_cnt[k] > 0) && (pf.recv_cnt[k] > 0) == (pc.recv_cnt[k] > 0), "%s: peer %d trades faces but not cells (or the reverse)", who.c_str(), pf.peers[k]);
		}
		for (size_t i = 0; i < t.up_foff.size() && t.up_off.size() == t.up_foff.size(); i++) {
			if (i > 0) CHECK(t.up_foff[i] > t.up_foff[i - 1] && t.up_off[i] > t.up_off[i - 1], "%s: up block %zu out of order", who.c_str(), i);
			if (t.repl_up) continue; // (every block goes to every peer)
			bool several = false;
			const int kc = rangeOf(pc.send_off, pc.send_cnt, t.up_off[i], &several), kf = rangeOf(pf.send_off, pf.send_cnt, t.up_foff[i], &several);
			CHECK(kc >= 0 && kc == kf && !several, "%s: up block %zu goes to peer %d as cells and %d as faces", who.c_str(), i, kc, kf);
		}
		for (size_t i = 0; i < t.down_foff.size() && t.down_off.size() == t.down_foff.size(); i++) {
			if (i > 0) CHECK(t.down_foff[i] > t.down_foff[i - 1] && t.down_off[i] > t.down_off[i - 1], "%s: down block %zu out of order", who.c_str(), i);
			bool several = false;
			const int kc = rangeOf(pc.recv_off, pc.recv_cnt, t.down_off[i], &several), kf = rangeOf(pf.recv_off, pf.recv_cnt, t.down_foff[i], &several);
			CHECK(kc >= 0 && kc == kf && !several, "%s: down block %zu comes from peer %d as cells and %d as faces", who.c_str(), i, kc, kf);
		}
	}
	// what r sends to q is what q expects from r
	for (int r = 0; r < R; r++)
		for (int q = 0; q < R; q++) {
			if (r == q) continue;
			const LevelTables &tr = T[r], &tq = T[q];
			const Level       &lr = H[r].levels[li], &cq = H[q].levels[li + 1];
			const size_t kr = std::find(tr.tx_fup.peers.begin(), tr.tx_fup.peers.end(), q) - tr.tx_fup.peers.begin();
			const size_t kq = std::find(tq.tx_fup.peers.begin(), tq.tx_fup.peers.end(), r) - tq.tx_fup.peers.begin();
			const int64_t sent = kr < tr.tx_fup.peers.size() ? tr.tx_fup.send_cnt[kr] : 0, want = kq < tq.tx_fup.peers.size() ? tq.tx_fup.recv_cnt[kq] : 0;
			CHECK(sent == want, "rank %d sends %lld doubles to %d, which expects %lld", r, (long long) sent, q, (long long) want);
			if (sent != want || sent == 0) continue;
			std::vector<Msg> out, in;
			const int64_t    s0 = tr.tx_fup.send_off[kr], r0 = tq.tx_fup.recv_off[kq];
			for (size_t i = 0; i < tr.up_foff.size(); i++)
				if (tr.up_foff[i] >= s0 && tr.up_foff[i] < s0 + sent)
					out.push_back({lr.g_parent[lr.l2g[tr.up_desc[2 * i]]], tr.up_desc[2 * i + 1], tr.up_foff[i] - s0});
			for (size_t j = 0; j < tq.down_foff.size(); j++)
				if (tq.down_foff[j] >= r0 && tq.down_foff[j] < r0 + want) in.push_back({cq.l2g[tq.down_desc[2 * j]], tq.down_desc[2 * j + 1], tq.down_foff[j] - r0});
			g_blocks += (long) out.size();
			for (auto &m : out) g_copy_blocks += m.o < 0;
			CHECK(out == in, "rank %d -> %d: %zu blocks sent, %zu expected, or another (parent, orthant, place) sequence", r, q, out.size(), in.size());
		}
	// on the receiving rank: every child of a local coarse patch has exactly one source
	for (int q = 0; q < R; q++) {
		const LevelTables &t = T[q];
		const Level       &lv = H[q].levels[li], &cv = H[q].levels[li + 1];
		std::vector<int>   used(t.down_foff.size(), 0);
		for (int gf = 0; gf < lv.P_global; gf++) {
			const int gpar = lv.g_parent[gf], o = lv.g_orth_on_parent[gf];
			if (cv.g_rank[gpar] != q) continue;
			const int e = t.child[(size_t) cv.g_local[gpar] * NCH + std::max(o, 0)];
			if (lv.g_rank[gf] == q) {
				CHECK(e == lv.g_local[gf], "rank %d: local child %d of coarse patch %d is filed as %d", q, gf, gpar, e);
				continue;
			}
			const int b = -(e + 2);
			CHECK(e <= -2 && b < (int) used.size(), "rank %d: remote child %d of coarse patch %d is filed as %d", q, gf, gpar, e);
			if (e > -2 || b >= (int) used.size()) continue;
			used[b]++;
			CHECK(t.down_desc[2 * b] == cv.g_local[gpar] && t.down_desc[2 * b + 1] == o, "rank %d: block %d is not child %d of coarse patch %d", q, b, o, gpar);
			bool      several = false;
			const int k       = rangeOf(t.tx_fup.recv_off, t.tx_fup.recv_cnt, t.down_foff[b], &several);
			CHECK(k >= 0 && !several && t.tx_fup.peers[k] == lv.g_rank[gf], "rank %d: block %d does not come from the child's rank %d", q, b, lv.g_rank[gf]);
		}
		for (size_t b = 0; b < used.size(); b++) CHECK(used[b] == 1, "rank %d: received block %zu is read %d times", q, b, used[b]);
		g_repl_levels += t.repl_up;
		if (t.repl_up) CHECK(cv.P == cv.P_global, "rank %d: repl_up towards a level that is not whole here", q);
	}
}

static int runCase(const Tree &tree, int n, int nranks, const Placement &pl)
{
	std::vector<Hierarchy> H;
	for (int r = 0; r < nranks; r++) H.push_back(Hierarchy::build(tree, n, false, 0, 0.0, r, nranks, pl));
	const std::string base = g_case;
	for (int li = 0; li + 1 < (int) H[0].levels.size(); li++) {
		std::vector<LevelTables> T(nranks);
		bool                     ok = true;
		g_case                      = base + " level " + std::to_string(li);
		for (int r = 0; r < nranks; r++) {
			const int rc = computeLevelTables(H[r], li, LevelBuildOpts(), T[r]);
			CHECK(rc == TE_OK, "computeLevelTables failed on rank %d", r);
			ok &= rc == TE_OK;
		}
		if (ok) checkLevel(H, T, li);
	}
	g_case = base;
	return 1;
}

int main(int argc, char **argv)
{
	if (argc != 2) return fprintf(stderr, "usage: %s <mesh directory>\n", argv[0]), 2;
	const struct {
		const char *file;
		int         dim, divides, n;
	} meshes[] = {{"2uni.bin", 3, 1, 8},          {"2refine.bin", 3, 1, 8},  {"multi_refine_8.bin", 3, 0, 4}, {"2d2uni.bin", 2, 2, 8},
	              {"2d2ref.bin", 2, 2, 8},        {"2d2ref.bin", 2, 1, 6},   {"2d_multi_refine_8.bin", 2, 0, 8}};
	// the small levels spread over the ranks, gathered on rank 0, and replicated on every rank
	const Placement placements[3] = {{0.0, -1, 0}, {16.0, -1, 0}, {16.0, -1, 1}};
	int             cases = 0;
	for (auto &m : meshes) {
		Tree tree = Tree::read(std::string(argv[1]) + "/" + m.file, m.dim);
		for (int d = 0; d < m.divides; d++) tree.refineLeaves();
		for (int nranks : {1, 2, 3, 4, 8})
			for (int ip = 0; ip < (nranks == 1 ? 1 : 3); ip++) {
				g_case = std::string(m.file) + " divides " + std::to_string(m.divides) + " n " + std::to_string(m.n) + " ranks " + std::to_string(nranks) + " placement "
				         + std::to_string(ip);
				cases += runCase(tree, m.n, nranks, placements[ip]);
			}
	}
	if (g_failures) return fprintf(stderr, "%d checks failed\n", g_failures), 1;
	if (g_blocks == 0 || g_copy_blocks == 0 || g_repl_levels == 0) return fprintf(stderr, "the meshes reach no travelling block, no copy-through block or no replicated level\n"), 1;
	printf("OK %d cases, %ld blocks between ranks (%ld copy through), %ld rank-levels under repl_up\n", cases, g_blocks, g_copy_blocks, g_repl_levels);
	return 0;
}
