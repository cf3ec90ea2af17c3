// The transfer of a level-0 face vector between the solvers of two meshes that are one te_mesh_adapt apart, te_faces_regrid
// (see gmg_internal.hpp). The kernels are in faceregridkernels.hpp; the map of destination patches and its
// device buffer are te_vec_regrid's (gmg_regrid.hip). No counterpart in the reference; nothing a cycle reads changes.
#include "gmg_ghosts3d.hpp"
#include "faceregridkernels.hpp" // (last: it switches FMA contraction off for what follows)

namespace tei
{
template <int N> static void faceRegridN(te_gmg *g, LevelHost &L, const int32_t *map, const double *hsrc, const double *src, double *dst)
{
	const int zs = stencilSlabs<N>(g, L.P);
	Timed     t(g, KC_FACE_REGRID, (size_t) L.P * L.nc);
	dispatchSlabs<N>(zs, [&](auto z) {
		hipLaunchKernelGGL((k_facexfer3d<N, decltype(z)::value>), slabGrid(L.P, zs), dim3(Tile3<N>::TPB), 0, g->stream, L.P, map, hsrc, src, dst);
	});
}

static int checkFaces0(te_gmg *g, const te_vec *v)
{
	if (!v) return te::fail(TE_EINVAL, "te_faces_regrid: null vector");
	if (v->g != g || v->level != 0) return te::fail(TE_EINVAL, "te_faces_regrid: vector does not belong to level 0 of its solver");
	if (!v->faces) return te::fail(TE_EINVAL, "te_faces_regrid: a face vector is needed (te_vec_create_faces); domain vectors travel through te_vec_regrid");
	return TE_OK;
}
} // namespace tei

extern "C" {
int te_faces_regrid(te_gmg *src, const te_vec *U_src, te_gmg *dst, te_vec *U_dst)
{
	return guarded([&]() -> int {
		int rc;
		if (!src || !dst) return te::fail(TE_EINVAL, "te_faces_regrid: null solver");
		if (src->nranks > 1 || dst->nranks > 1)
			return te::fail(TE_ESTATE, "te_faces_regrid: not implemented on a sharded hierarchy (source patches on another rank would have to travel)");
		if ((rc = checkFaces0(src, U_src)) || (rc = checkFaces0(dst, U_dst))) return rc;
		if (src->dim != dst->dim || src->n != dst->n)
			return te::fail(TE_EINVAL, "te_faces_regrid: the two solvers differ in dim or n (" + std::to_string(src->dim) + "D n = " + std::to_string(src->n)
			                               + " and " + std::to_string(dst->dim) + "D n = " + std::to_string(dst->n) + ")");
		if (src->device != dst->device) return te::fail(TE_EINVAL, "te_faces_regrid: the two solvers live on different devices");
		if (U_src == U_dst) return te::fail(TE_EINVAL, "te_faces_regrid: source and destination are the same vector");
		LevelHost &L = *dst->levels[0];
		if (L.P == 0) return TE_OK;
		const int32_t *map = nullptr;
		if ((rc = regridMapUpload(src, dst, "te_faces_regrid", &map))) return rc;
		const double *hsrc = src->levels[0]->geom_h.p; // [P_src][3]: the refinement's h_a / h_b
		if (L.dim == 2) {
			Timed t(dst, KC_FACE_REGRID, (size_t) L.P * L.nc);
			hipLaunchKernelGGL(k_facexfer2d, dim3(gridFor((size_t) L.P * L.nc / 2, 256, 65536)), dim3(256), 0, dst->stream, L.n, L.P, map, hsrc, U_src->d,
			                   U_dst->d);
		} else {
			dispatchN(L.n, [&](auto n) { faceRegridN<decltype(n)::value>(dst, L, map, hsrc, U_src->d, U_dst->d); });
		}
		HIPCHK(hipGetLastError());
		return TE_OK;
	});
}
} // extern "C"
