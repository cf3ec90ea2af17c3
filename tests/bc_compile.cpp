// CPU, syntax only: a driver with one IsNeumann per side, written against the reference's Vector<D> interface, sets
// LevelGeometry::neumann_sides and fills f / exact through tehip::initSides / initSides2d (thunderegg/HipInit.h).
// Compiled by tests/test_bc_dropin_compile.py against the reference's own headers; nothing is run.
#include <HipInit.h>
#include <cmath>

template <size_t D> void fillWithSides(const te_hier *h, const bool (&is_neumann)[2 * D], std::shared_ptr<Vector<D>> f, std::shared_ptr<Vector<D>> exact);

template <> void fillWithSides<3>(const te_hier *h, const bool (&is_neumann)[6], std::shared_ptr<Vector<3>> f, std::shared_ptr<Vector<3>> exact)
{
	tehip::LevelGeometry G(h, 0);
	int                  mask = 0;
	for (int s = 0; s < 6; s++) mask |= (is_neumann[s] ? 1 : 0) << s;
	if (G.neumann_sides != mask) throw 3; // (the hierarchy was built with te_hier_build_bc(.., mask, ..))
	auto e = [](double x, double y, double z) { return sin(x) * cos(y) * z; };
	auto r = [](double x, double y, double z) { return -2 * sin(x) * cos(y) * z; };
	tehip::initSides(G, f, exact, r, e, [](double x, double y, double z) { return cos(x) * cos(y) * z; },
	                 [](double x, double y, double z) { return -sin(x) * sin(y) * z; }, [](double x, double y, double) { return sin(x) * cos(y); });
}

template <> void fillWithSides<2>(const te_hier *h, const bool (&is_neumann)[4], std::shared_ptr<Vector<2>> f, std::shared_ptr<Vector<2>> exact)
{
	tehip::LevelGeometry G(h, 0);
	G.neumann_sides = 0;
	for (int s = 0; s < 4; s++) G.neumann_sides |= (is_neumann[s] ? 1 : 0) << s;
	auto e = [](double x, double y) { return sin(x) * cos(y); };
	auto r = [](double x, double y) { return -2 * sin(x) * cos(y); };
	tehip::initSides2d(G, f, exact, r, e, [](double x, double y) { return cos(x) * cos(y); }, [](double x, double y) { return -sin(x) * sin(y); });
}
