// CPU: te_mesh_adapt and what hangs on it (te_mesh_leaves, te_mesh_is_balanced, te_hier_build on the adapted trees, te_hier_leaf_tree)
// under AddressSanitizer + UndefinedBehaviorSanitizer, driven through include/te_hip.h. A stand-alone program over csrc/mesh.cpp and
// csrc/capi_mesh.cpp, built and run by tests/test_regrid_sanitize.py. Every fixture goes through three seeded adapts per pattern:
// random flags per leaf (ripples), random flags per family (families go), all +1, all -1.
#include "te_hip.h"
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

static int fail(const char *what)
{
	fprintf(stderr, "FAILED: %s: %s\n", what, te_last_error());
	return 1;
}

static uint64_t next(uint64_t &s) // splitmix64
{
	uint64_t z = (s += 0x9E3779B97F4A7C15ull);
	z          = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z          = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	return z ^ (z >> 31);
}

int main(int argc, char **argv)
{
	long leaves_seen = 0;
	for (int a = 1; a + 1 < argc; a += 2) { // pairs: mesh file, dim
		const int dim = atoi(argv[a + 1]);
		for (int pattern = 0; pattern < 4; pattern++) {
			te_mesh *m = nullptr;
			if (te_mesh_read(argv[a], dim, &m)) return fail("te_mesh_read");
			uint64_t seed = 1 + pattern;
			for (int step = 0; step < 3; step++) {
				const int nl = te_mesh_num_leaves(m), nn = te_mesh_num_nodes(m);
				if (nl <= 0) return fail("te_mesh_num_leaves");
				if (nl > 800) break; // (the sanitizers cost a factor of ten or more: the deep trees stop growing here)
				std::vector<int32_t> ids(nl), flags(nl), ilp((size_t) nn * 3);
				if (te_mesh_leaves(m, ids.data())) return fail("te_mesh_leaves");
				if (te_mesh_get_nodes(m, ilp.data(), nullptr, nullptr, nullptr, nullptr)) return fail("te_mesh_get_nodes");
				std::map<int, int> parent, pick;
				for (int i = 0; i < nn; i++) parent[ilp[3 * i]] = ilp[3 * i + 2];
				for (int i = 0; i < nl; i++) {
					if (pattern == 0) flags[i] = (int) (next(seed) % 3) - 1;
					if (pattern == 1) {
						auto it = pick.find(parent[ids[i]]);
						if (it == pick.end()) it = pick.emplace(parent[ids[i]], (int) (next(seed) % 3) - 1).first;
						flags[i] = it->second;
					}
					if (pattern >= 2) flags[i] = pattern == 2 ? 1 : -1;
				}
				te_mesh *out = nullptr;
				if (te_mesh_adapt(m, nl, ids.data(), flags.data(), &out)) return fail("te_mesh_adapt");
				if (te_mesh_is_balanced(out) != 1) return fail("the adapted tree is not balanced");
				const int no = te_mesh_num_leaves(out);
				for (int nranks : {1, 3}) {
					for (int rank = 0; rank < nranks; rank++) {
						te_hier *h = nullptr;
						if (te_hier_build(out, 4, 0, 0, 0.0, rank, nranks, &h)) return fail("te_hier_build");
						int pl = 0, pg = 0;
						if (te_hier_level_sizes(h, 0, &pl, &pg) || pg != no) return fail("level 0 does not hold the leaves");
						std::vector<int32_t> id(pg), par(pg), orth(pg);
						if (te_hier_leaf_tree(h, id.data(), par.data(), orth.data()) || te_hier_leaf_tree(h, nullptr, nullptr, nullptr))
							return fail("te_hier_leaf_tree");
						leaves_seen += pg;
						te_hier_destroy(h);
					}
				}
				te_mesh_destroy(m);
				m = out;
			}
			// error paths come back as codes: an unknown id, a duplicate, a bad flag, a node that is not a leaf
			const int            nl = te_mesh_num_leaves(m);
			std::vector<int32_t> ids(nl);
			if (te_mesh_leaves(m, ids.data())) return fail("te_mesh_leaves");
			te_mesh      *out = nullptr;
			const int32_t unknown[1] = {1 << 30}, twice[2] = {ids[0], ids[0]}, one[2] = {1, 1}, two[1] = {2};
			if (te_mesh_adapt(m, 1, unknown, one, &out) != TE_EINVAL) return fail("unknown id accepted");
			if (te_mesh_adapt(m, 2, twice, one, &out) != TE_EINVAL) return fail("duplicate accepted");
			if (te_mesh_adapt(m, 1, ids.data(), two, &out) != TE_EINVAL) return fail("flag 2 accepted");
			if (nl > 1) {
				std::vector<int32_t> ilp((size_t) te_mesh_num_nodes(m) * 3);
				if (te_mesh_get_nodes(m, ilp.data(), nullptr, nullptr, nullptr, nullptr)) return fail("te_mesh_get_nodes");
				const int32_t inner[1] = {ilp[2 + 3 * (ilp.size() / 3 - 1)]}; // the last node's parent
				if (te_mesh_adapt(m, 1, inner, one, &out) != TE_EINVAL) return fail("a node with children accepted");
			}
			te_mesh_destroy(m);
		}
	}
	printf("SANITIZE_OK %ld\n", leaves_seen);
	return 0;
}
