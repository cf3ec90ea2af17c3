// CPU: the boundary entry points of the host-only half of the C ABI (te_hier_build_bc, te_hier_neumann_sides, te_hier_singular,
// te_hier_num_bfaces, te_hier_bface_index) under AddressSanitizer + UndefinedBehaviorSanitizer, driven through include/te_hip.h.
// Built and run by tests/test_bc_host.py.
#include "te_hip.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

static int fail(const char *what)
{
	fprintf(stderr, "FAILED: %s: %s\n", what, te_last_error());
	return 1;
}

int main(int argc, char **argv)
{
	long faces = 0;
	for (int a = 1; a + 2 < argc; a += 3) { // triples: mesh file, dim, divides
		const int dim = atoi(argv[a + 1]), div = atoi(argv[a + 2]), ns = 2 * dim, all = (1 << ns) - 1;
		te_mesh  *m = nullptr;
		if (te_mesh_read(argv[a], dim, &m)) return fail("te_mesh_read");
		for (int i = 0; i < div; i++)
			if (te_mesh_refine_leaves(m)) return fail("te_mesh_refine_leaves");
		for (int mask : {0, 5, all - 1, all}) {
			for (int nranks : {1, 2, 3, 8}) {
				for (int rank = 0; rank < nranks; rank++) {
					te_hier *h = nullptr;
					if (te_hier_build_bc(m, 4, mask, 0, 0.0, rank, nranks, -1.0, -1, rank & 1, &h)) return fail("te_hier_build_bc");
					if (te_hier_neumann_sides(h) != mask || te_hier_singular(h) != (mask == all)) return fail("mask round trip");
					for (int l = 0; l < te_hier_num_levels(h); l++) {
						int pl = 0, pg = 0, nb = -1;
						if (te_hier_level_sizes(h, l, &pl, &pg) || te_hier_num_bfaces(h, l, &nb)) return fail("te_hier_num_bfaces");
						std::vector<int32_t> idx((size_t) pl * ns, -7);
						if (te_hier_bface_index(h, l, pl ? idx.data() : nullptr)) return fail("te_hier_bface_index");
						int next = 0;
						for (int32_t v : idx) {
							if (v != -1 && v != next) return fail("bface numbering");
							next += v >= 0;
						}
						if (next != nb) return fail("bface count");
						faces += nb;
					}
					te_hier_destroy(h);
				}
			}
		}
		// error paths: codes, not exceptions or leaks
		te_hier *h = nullptr;
		int      nb = 0;
		if (te_hier_build_bc(m, 4, all + 1, 0, 0.0, 0, 1, -1.0, -1, -1, &h) != TE_EINVAL) return fail("bit above 2 dim accepted");
		if (te_hier_build_bc(m, 4, -1, 0, 0.0, 0, 1, -1.0, -1, -1, &h) != TE_EINVAL) return fail("negative mask accepted");
		if (te_hier_build_bc(m, 7, 1, 0, 0.0, 0, 1, -1.0, -1, -1, &h) == TE_OK) return fail("odd n accepted");
		if (te_hier_build_bc(m, 4, 1, 0, 0.0, 0, 1, -1.0, -1, -1, &h)) return fail("te_hier_build_bc");
		if (te_hier_num_bfaces(h, 99, &nb) != TE_EINVAL || te_hier_bface_index(h, -1, nullptr) != TE_EINVAL) return fail("bad level accepted");
		if (te_hier_neumann_sides(nullptr) >= 0 || te_hier_singular(nullptr) >= 0) return fail("null hierarchy accepted");
		te_hier_destroy(h);
		te_mesh_destroy(m);
	}
	printf("SANITIZE_OK %ld\n", faces);
	return 0;
}
