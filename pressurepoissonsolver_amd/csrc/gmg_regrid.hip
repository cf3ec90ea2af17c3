// Regridding (see gmg_internal.hpp): the per-patch indicator te_patch_indicator and the transfer of a level-0
// vector between the solvers of two meshes that are one te_mesh_adapt apart, te_vec_regrid. The kernels are in regridkernels.hpp.
// Neither call has a counterpart in the reference, and neither changes anything a cycle reads.
#include "gmg_ghosts3d.hpp"
#include "regridkernels.hpp"

// the indicator's per-slab and per-patch values on the device, and the transfer's map (one row per destination patch)
struct RegridWs {
	DevBuf<double>  part, out;
	DevBuf<int32_t> map;
};

namespace tei
{
void regridFree(te_gmg *g)
{
	delete g->regrid;
	g->regrid = nullptr;
}

static RegridWs &regridWs(te_gmg *g)
{
	if (!g->regrid) g->regrid = new RegridWs;
	return *g->regrid;
}

template <int N> static void indicatorN(te_gmg *g, LevelHost &L, const double *u, RegridWs &W)
{
	const int zs = stencilSlabs<N>(g, L.P);
	Timed     t(g, KC_INDICATOR, (size_t) L.P * L.nc);
	double   *first = zs == 1 ? W.out.p : W.part.p;
	dispatchSlabs<N>(zs, [&](auto z) {
		hipLaunchKernelGGL((k_indicator3d<N, decltype(z)::value>), dim3(L.P * zs), dim3(256), 0, g->stream, L.P, u, first);
	});
	if (zs > 1) hipLaunchKernelGGL(k_indicator_final, dim3((L.P + 255) / 256), dim3(256), 0, g->stream, L.P, zs, W.part.p, W.out.p);
}

template <int N> static void regridN(te_gmg *g, LevelHost &L, const int32_t *map, const double *src, double *dst)
{
	const int zs = stencilSlabs<N>(g, L.P);
	Timed     t(g, KC_REGRID, (size_t) L.P * L.nc);
	dispatchSlabs<N>(zs, [&](auto z) {
		hipLaunchKernelGGL((k_regrid3d<N, decltype(z)::value>), slabGrid(L.P, zs), dim3(Tile3<N>::TPB), 0, g->stream, L.P, map, src, dst);
	});
}

// One row per destination patch from the two solvers' leaf tables. A match by node id is confirmed by position and size: ids are
// reused once a node has been removed, so two meshes further apart than one adapt step could agree on an id and mean another box.
static int regridMap(const te_gmg *src, const te_gmg *dst, const char *who, std::vector<int32_t> &map)
{
	const int dim = dst->dim, north = 1 << dim, Pd = (int) dst->leaf_id.size(), Ps = (int) src->leaf_id.size();
	std::map<int, int>              leaf;     // source node id -> source patch
	std::map<int, std::vector<int>> children; // source tree parent -> its leaf children, by orthant
	for (int p = 0; p < Ps; p++) {
		leaf[src->leaf_id[p]] = p;
		if (src->leaf_parent[p] >= 0) {
			auto &c = children[src->leaf_parent[p]];
			if (c.empty()) c.assign(north, -1);
			c[src->leaf_orth[p]] = p;
		}
	}
	auto S = [&](int p, int a) { return src->leaf_starts[(size_t) p * dim + a]; };
	auto SL = [&](int p, int a) { return src->leaf_lengths[(size_t) p * dim + a]; };
	auto D = [&](int p, int a) { return dst->leaf_starts[(size_t) p * dim + a]; };
	auto DL = [&](int p, int a) { return dst->leaf_lengths[(size_t) p * dim + a]; };
	// The child's box as Tree::refineNode computes it from the parent's, and equal boxes, up to rounding: a mesh file may hold boxes
	// that were halved in another order. 1e-9 of the box's length is far below one cell and far above any rounding.
	auto near = [](double a, double b, double len) { return std::fabs(a - b) <= 1e-9 * std::fabs(len); };
	auto childOf = [&](double ps, double pl, int upper, double cs, double cl) { return near(cl, pl / 2, pl) && near(cs, upper ? ps + pl / 2 : ps, pl); };
	map.assign((size_t) Pd * RG_ROW, -1);
	for (int p = 0; p < Pd; p++) {
		int32_t *row = map.data() + (size_t) p * RG_ROW;
		const int id = dst->leaf_id[p];
		bool      ok = false;
		auto      it = leaf.find(id);
		if (it != leaf.end()) {
			ok = true;
			for (int a = 0; a < dim; a++) ok = ok && near(S(it->second, a), D(p, a), DL(p, a)) && near(SL(it->second, a), DL(p, a), DL(p, a));
			row[0] = RG_COPY, row[1] = -1, row[2] = it->second;
		} else if (dst->leaf_parent[p] >= 0 && (it = leaf.find(dst->leaf_parent[p])) != leaf.end()) {
			const int o = dst->leaf_orth[p];
			ok          = true;
			for (int a = 0; a < dim; a++) ok = ok && childOf(S(it->second, a), SL(it->second, a), (o >> a) & 1, D(p, a), DL(p, a));
			row[0] = RG_REFINE, row[1] = o, row[2] = it->second;
		} else {
			auto ch = children.find(id);
			if (ch != children.end()) {
				ok = true;
				for (int o = 0; o < north && ok; o++) {
					const int c = ch->second[o];
					ok          = c >= 0;
					for (int a = 0; a < dim && ok; a++) ok = childOf(D(p, a), DL(p, a), (o >> a) & 1, S(c, a), SL(c, a));
					row[2 + o] = c;
				}
				row[0] = RG_COARSEN, row[1] = -1;
			}
		}
		if (!ok)
			return te::fail(TE_EINVAL, std::string(who) + ": destination leaf with node id " + std::to_string(id)
			                               + " has no source: it is neither a source leaf, nor the child of one, nor the parent of 2^dim source "
			                                 "leaves in the same place (the two meshes must be one te_mesh_adapt apart)");
	}
	return TE_OK;
}

// the map of a transfer from src to dst on the device, in dst's buffer (te_vec_regrid and te_faces_regrid share it); both streams
// are synchronised: src's, whose results the transfer reads, and dst's, where an earlier transfer may still read the map that is
// replaced or overwritten here
int regridMapUpload(te_gmg *src, te_gmg *dst, const char *who, const int32_t **map_dev)
{
	int                  rc;
	std::vector<int32_t> map;
	if ((rc = regridMap(src, dst, who, map))) return rc;
	HIPCHK(hipSetDevice(dst->device));
	HIPCHK(hipStreamSynchronize(src->stream));
	RegridWs &W = regridWs(dst);
	HIPCHK(hipStreamSynchronize(dst->stream));
	if (W.map.n < map.size() && (rc = W.map.alloc(map.size()))) return rc;
	HIPCHK(hipMemcpy(W.map.p, map.data(), sizeof(int32_t) * map.size(), hipMemcpyHostToDevice));
	*map_dev = W.map.p;
	return TE_OK;
}
} // namespace tei

extern "C" {
int te_patch_indicator(te_gmg *g, int level, const te_vec *u, double *out_host)
{
	return guarded([&]() -> int {
		int rc;
		if ((rc = checkLevelVec(g, level, u, "te_patch_indicator"))) return rc;
		LevelHost &L = *g->levels[level];
		if (L.P == 0) return TE_OK;
		if (!out_host) return te::fail(TE_EINVAL, "te_patch_indicator: null output");
		RegridWs &W = regridWs(g);
		if (W.out.n < (size_t) L.P && (rc = W.out.alloc((size_t) L.P))) return rc;
		if (W.part.n < (size_t) L.P * 8 && (rc = W.part.alloc((size_t) L.P * 8))) return rc; // (at most 8 slabs per patch)
		if (L.dim == 2) {
			Timed t(g, KC_INDICATOR, (size_t) L.P * L.nc);
			hipLaunchKernelGGL(k_indicator2d, dim3(L.P), dim3(256), 0, g->stream, L.n, L.P, u->d, W.out.p);
		} else {
			dispatchN(L.n, [&](auto n) { indicatorN<decltype(n)::value>(g, L, u->d, W); });
		}
		HIPCHK(hipGetLastError());
		HIPCHK(hipStreamSynchronize(g->stream));
		HIPCHK(hipMemcpy(out_host, W.out.p, sizeof(double) * L.P, hipMemcpyDeviceToHost));
		return TE_OK;
	});
}

int te_vec_regrid(te_gmg *src, const te_vec *u_src, te_gmg *dst, te_vec *u_dst)
{
	return guarded([&]() -> int {
		int rc;
		if (!src || !dst) return te::fail(TE_EINVAL, "te_vec_regrid: null solver");
		if (src->nranks > 1 || dst->nranks > 1)
			return te::fail(TE_ESTATE, "te_vec_regrid: not implemented on a sharded hierarchy (source patches on another rank would have to travel)");
		if ((rc = checkLevelVec(src, 0, u_src, "te_vec_regrid")) || (rc = checkLevelVec(dst, 0, u_dst, "te_vec_regrid"))) return rc;
		if (src->dim != dst->dim || src->n != dst->n)
			return te::fail(TE_EINVAL, "te_vec_regrid: the two solvers differ in dim or n (" + std::to_string(src->dim) + "D n = " + std::to_string(src->n)
			                               + " and " + std::to_string(dst->dim) + "D n = " + std::to_string(dst->n) + ")");
		if (src->device != dst->device) return te::fail(TE_EINVAL, "te_vec_regrid: the two solvers live on different devices");
		if (u_src == u_dst) return te::fail(TE_EINVAL, "te_vec_regrid: source and destination are the same vector");
		LevelHost &L = *dst->levels[0];
		if (L.P == 0) return TE_OK;
		const int32_t *map = nullptr;
		if ((rc = regridMapUpload(src, dst, "te_vec_regrid", &map))) return rc;
		if (L.xf_valid_for == u_dst->d) L.xf_valid_for = nullptr; // u_dst is overwritten
		if (L.dim == 2) {
			Timed t(dst, KC_REGRID, (size_t) L.P * L.nc);
			hipLaunchKernelGGL(k_regrid2d, dim3(gridFor((size_t) L.P * L.nc / 2, 256, 65536)), dim3(256), 0, dst->stream, L.n, L.P, map, u_src->d,
			                   u_dst->d);
		} else {
			dispatchN(L.n, [&](auto n) { regridN<decltype(n)::value>(dst, L, map, u_src->d, u_dst->d); });
		}
		HIPCHK(hipGetLastError());
		return TE_OK;
	});
}
} // extern "C"
