// Face vectors and the MAC operators on them: gradient of a cell vector, divergence of a face vector, pressure projection
// (projkernels.hpp; see gmg_internal.hpp). The gradient and the projection make the level's ghosts current exactly as te_apply
// does (withGhosts / prepareGhosts2d): collective on a sharded hierarchy. The divergence reads only its own patches.
#include "gmg_ghosts3d.hpp"
#include "projkernels.hpp"

namespace tei
{
static int checkFaceVec(te_gmg *g, int level, const te_vec *v, const char *who)
{
	if (!g || !v || level < 0 || level >= (int) g->levels.size() || v->g != g || v->level != level || !v->faces)
		return te::fail(TE_EINVAL, std::string(who) + ": not a face vector of this level");
	return TE_OK;
}
static int checkBdata(te_gmg *g, int level, const te_vec *v, const char *who)
{
	if (v && (!g || v->g != g || v->level != level || !v->bnd)) return te::fail(TE_EINVAL, std::string(who) + ": bdata is not a boundary vector of this level");
	return TE_OK;
}

static int faceGeom(LevelHost &L, const te_vec *bdata, FaceGeom *F)
{
	int rc;
	F->h = L.geom_h.p, F->bface = nullptr, F->bdata = nullptr;
	if (!bdata || L.nbf == 0) return TE_OK;
	if (!L.bface.p && !L.bface_host.empty() && (rc = L.bface.upload(L.bface_host))) return rc;
	F->bface = L.bface.p, F->bdata = bdata->d;
	return TE_OK;
}

template <int N, bool PROJECT> static int gradientN(te_gmg *g, LevelHost &L, const FaceGeom &F, const double *u, double *G, double alpha)
{
	const int zs     = stencilSlabs<N>(g, L.P);
	auto      launch = [&](LevelDev D) {
		if (D.count == 0) return;
		Timed t(g, PROJECT ? KC_PROJECT : KC_GRADIENT, (size_t) D.count * L.nc);
		dispatchSlabs<N>(zs, [&](auto z) {
			hipLaunchKernelGGL((k_gradient3d<N, PROJECT, decltype(z)::value>), slabGrid(D.count, zs), dim3(Tile3<N>::TPB), 0, g->stream, D, F, u, G,
			                   alpha);
		});
	};
	int rc = withGhosts<N>(g, L, {u}, launch);
	if (rc) return rc;
	HIPCHK(hipGetLastError());
	return TE_OK;
}

template <bool PROJECT> static int gradient(te_gmg *g, LevelHost &L, const te_vec *u, const te_vec *bdata, te_vec *G, double alpha)
{
	if (L.P == 0) return TE_OK;
	FaceGeom F;
	int      rc = faceGeom(L, bdata, &F);
	if (rc) return rc;
	if (L.dim == 2) {
		if ((rc = prepareGhosts2d(g, L, u->d))) return rc;
		Timed t(g, PROJECT ? KC_PROJECT : KC_GRADIENT, (size_t) L.P * L.nc);
		hipLaunchKernelGGL(k_gradient2d<PROJECT>, dim3(gridFor((size_t) L.P * L.nc / 2, 256, 65536)), dim3(256), 0, g->stream, L.dev2(), F,
		                   (const double *) u->d, G->d, alpha);
		HIPCHK(hipGetLastError());
		return TE_OK;
	}
	return dispatchN(L.n, [&](auto n) { return gradientN<decltype(n)::value, PROJECT>(g, L, F, u->d, G->d, alpha); });
}

template <int N> static void divergenceN(te_gmg *g, LevelHost &L, const double *U, double *out, double alpha)
{
	const int zs = stencilSlabs<N>(g, L.P);
	dispatchSlabs<N>(zs, [&](auto z) {
		hipLaunchKernelGGL((k_divergence3d<N, decltype(z)::value>), slabGrid(L.P, zs), dim3(Tile3<N>::TPB), 0, g->stream, L.P, L.geom_h.p, U, out,
		                   alpha);
	});
}
} // namespace tei

extern "C" {
int te_vec_create_faces(te_gmg *g, int level, te_vec **out)
{
	return guarded([&]() -> int {
		if (!g || !out || level < 0 || level >= (int) g->levels.size()) return te::fail(TE_EINVAL, "te_vec_create_faces: bad argument");
		LevelHost &L = *g->levels[level];
		HIPCHK(hipSetDevice(g->device));
		auto v   = std::make_unique<te_vec>();
		v->g     = g;
		v->level = level;
		v->faces = true;
		v->n     = (size_t) L.P * ((size_t) L.dim * L.nc + (size_t) L.dim * L.nf);
		HIPCHK(hipMalloc(&v->d, sizeof(double) * std::max<size_t>(v->n, 2)));
		hipError_t e = hipMemsetAsync(v->d, 0, sizeof(double) * v->n, g->stream);
		if (e != hipSuccess) {
			(void) hipFree(v->d);
			return te::fail(TE_EHIP, std::string("hipMemsetAsync: ") + hipGetErrorString(e));
		}
		*out = v.release();
		return TE_OK;
	});
}

int te_gradient(te_gmg *g, int level, const te_vec *u, const te_vec *bdata, te_vec *G)
{
	return guarded([&]() -> int {
		int rc;
		if ((rc = checkLevelVec(g, level, u, "te_gradient")) || (rc = checkBdata(g, level, bdata, "te_gradient"))
		    || (rc = checkFaceVec(g, level, G, "te_gradient")))
			return rc;
		return gradient<false>(g, *g->levels[level], u, bdata, G, 0.0);
	});
}

int te_project(te_gmg *g, int level, double alpha, const te_vec *p, const te_vec *bdata, te_vec *U)
{
	return guarded([&]() -> int {
		int rc;
		if ((rc = checkLevelVec(g, level, p, "te_project")) || (rc = checkBdata(g, level, bdata, "te_project"))
		    || (rc = checkFaceVec(g, level, U, "te_project")))
			return rc;
		return gradient<true>(g, *g->levels[level], p, bdata, U, alpha);
	});
}

int te_divergence(te_gmg *g, int level, double alpha, const te_vec *U, te_vec *out)
{
	return guarded([&]() -> int {
		int rc;
		if ((rc = checkFaceVec(g, level, U, "te_divergence")) || (rc = checkLevelVec(g, level, out, "te_divergence"))) return rc;
		LevelHost &L = *g->levels[level];
		if (L.P == 0) return TE_OK;
		if (L.xf_valid_for == out->d) L.xf_valid_for = nullptr; // out changes
		Timed t(g, KC_DIVERGENCE, (size_t) L.P * L.nc);
		if (L.dim == 2) {
			hipLaunchKernelGGL(k_divergence2d, dim3(gridFor((size_t) L.P * L.nc / 2, 256, 65536)), dim3(256), 0, g->stream, L.P, L.n, L.geom_h.p,
			                   (const double *) U->d, out->d, alpha);
		} else {
			dispatchN(L.n, [&](auto n) { divergenceN<decltype(n)::value>(g, L, U->d, out->d, alpha); });
		}
		HIPCHK(hipGetLastError());
		return TE_OK;
	});
}
} // extern "C"
