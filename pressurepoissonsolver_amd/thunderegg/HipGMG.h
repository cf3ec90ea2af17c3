// Header-only C++ adaptors that put the MI355X path (libte_hip.so, include/te_hip.h) behind the
// reference's own plugin surface, so GMG::Cycle<D>, BiCGStab<D> and apps/3d/steady.cpp run
// unchanged on device-resident vectors. Compiles against the reference's headers
// (-I$THUNDEREGG_REF/src): every class below derives from a reference interface.
//
//   HipVector<D>       : Vector<D>            (Vector.h:179-322)  all BLAS-1 virtuals overridden
//   HipVG<D>           : VectorGenerator<D>   (Vector.h:323-327)
//   HipOperator<D>     : Operator<D>          (Operators/Operator.h:28-38)   == SchurDomainOp / DomainWrapOp
//   HipSmoother<D>     : GMG::Smoother<D>     (GMG/Smoother.h:39)            == FFTBlockJacobiSmoother (kind 0)
//   HipRestrictor<D>   : GMG::Restrictor<D>   (GMG/Restrictor.h:39-40)       == AvgRstr
//   HipInterpolator<D> : GMG::Interpolator<D> (GMG/Interpolator.h:39-40)     == DrctIntp
//   HipLinearInterpolator<D> : GMG::Interpolator<D>                            stands behind TriLinIntp (te_prolong_linear_add; single rank)
//   HipCycle<D>        : Operator<D>          whole GMG::Cycle<D>::apply (GMG/Cycle.h:116-126) in one call
// The Schur-complement route (--schur, apps/3d/steady.cpp:336-420, apps/2d/steady.cpp:383-480; single rank):
//   HipSchurVG<D>      : VectorGenerator<D-1> SchurHelper<D>::getNewSchurVec (SchurHelper.h:156-160): HipVector<D-1> over
//                                             an interface vector, one "patch" per interface block of n^(D-1) values
//   HipSchurOp<D>      : Operator<D-1>        y = x - T x, the Schur operator (Operators/SchurWrapOp.h with its identity
//                                             term); rhs() = g = Interp(Solve(f, 0)), solution() = u = Solve(f, gamma)
//   HipChebPrec<D>     : Operator<D-1>        PolyChebPrec::apply (PolyChebPrec.cpp)
// The MAC operators of a projection step (te_gradient / te_divergence / te_project; they replace nothing in the reference):
//   HipFaceVector<D>   : (no base)            RAII face vector (te_vec_create_faces), host transfer by whole patches
//   gradient / divergence / project           free functions taking HipVector<D> and HipFaceVector<D>
//
// Error convention: the reference throws `int` (`throw 3;`, e.g. GMG/InterLevelComm.h:175,
// SchurHelper.h:129); a non-zero te_* status is rethrown the same way.
// Ownership: everything by std::shared_ptr, as the reference does (GMG/Level.h:84-186 setters).
// Threading: none; one solver stream per te_gmg; not re-entrant (same as the reference).
#ifndef THUNDEREGG_HIP_GMG_H
#define THUNDEREGG_HIP_GMG_H
#include <Thunderegg/GMG/Interpolator.h>
#include <Thunderegg/GMG/Restrictor.h>
#include <Thunderegg/GMG/Smoother.h>
#include <Thunderegg/Operators/Operator.h>
#include <Thunderegg/Vector.h>
#include <map>
#include <memory>
#include <te_hip.h>
#include <vector>

namespace tehip
{
inline void check(int status)
{
	if (status != TE_OK) throw 3; // the reference's error convention
}

/// Owns a te_gmg; shared by every adaptor created from it.
struct Context {
	te_gmg *g = nullptr;
	int     n = 0, dim = 0;
	explicit Context(const te_hier *h, int device = -1)
	{
		check(te_gmg_create(h, device, &g));
		n   = te_hier_n(h);
		dim = te_hier_dim(h);
	}
	~Context() { te_gmg_destroy(g); }
	Context(const Context &) = delete;
	Context &operator=(const Context &) = delete;
};

/// Host side of getLocalData(): ONE mirror per vector, shared by all the views handed out, holding only the patches
/// that are currently viewed. The first view of a patch downloads that patch (te_vec_download_patches: n^D doubles,
/// not the vector); further views of the same patch alias the same host memory, as every VecGetArray of a
/// PetscVector aliases the same storage (PetscVector.h:27-58), so concurrent views cannot lose each other's
/// updates; when the last view of a patch goes away and any of them was writable the patch is uploaded back.
struct HipMirror {
	te_vec *v;
	size_t  cells; // per patch
	struct Slot {
		std::vector<double> host;
		int                 views = 0;
		bool                dirty = false;
	};
	std::map<int, Slot> slots;
	int                 failed = 0; // status of the last failed write-back (a destructor cannot throw)
	HipMirror(te_vec *v_, size_t cells_) : v(v_), cells(cells_) {}
	double *acquire(int patch, bool writable)
	{
		Slot &s = slots[patch];
		if (s.views == 0) {
			s.host.resize(cells);
			check(te_vec_download_patches(v, patch, 1, s.host.data()));
		}
		s.views++;
		s.dirty |= writable;
		return s.host.data();
	}
	void release(int patch)
	{
		auto it = slots.find(patch);
		if (it == slots.end() || --it->second.views > 0) return;
		if (it->second.dirty) {
			int rc = te_vec_upload_patches(v, patch, 1, it->second.host.data());
			if (rc != TE_OK) failed = rc;
		}
		slots.erase(it);
	}
};
/// The manager a LocalData carries: releases its patch when the last copy of the view is gone (the role PetscLDM
/// plays for PetscVector).
class HipLDM : public LocalDataManager
{
	std::shared_ptr<HipMirror> mirror;
	int                        patch;

	public:
	double *data;
	HipLDM(std::shared_ptr<HipMirror> m, int patch_, bool writable) : mirror(m), patch(patch_), data(m->acquire(patch_, writable)) {}
	~HipLDM() { mirror->release(patch); }
};

template <size_t D> class HipVector : public Vector<D>
{
	public:
	std::shared_ptr<Context>   ctx;
	te_vec                    *v = nullptr;
	int                        level;
	std::shared_ptr<HipMirror> mirror;
	/// iface: an interface vector of a (D+1)-dimensional level (te_vec_create_iface): its "patches" are the interface blocks,
	/// n^D values each, in SchurHelper's local order
	HipVector(std::shared_ptr<Context> ctx_, int level_, bool iface = false) : ctx(ctx_), level(level_)
	{
		check(iface ? te_vec_create_iface(ctx->g, level, &v) : te_vec_create(ctx->g, level, &v));
		size_t cells = 1;
		for (size_t i = 0; i < D; i++) cells *= ctx->n;
		this->num_local_patches = (int) (te_vec_size(v) / cells);
		mirror.reset(new HipMirror(v, cells));
	}
	~HipVector()
	{
		mirror->v = nullptr; // (no view can outlive the vector: LocalData is used inside patch loops)
		te_vec_destroy(v);
	}
	/// status of the last failed write-back of a released view, TE_OK if none (a destructor cannot throw)
	int writeBackStatus() const { return mirror->failed; }
	static const te_vec *raw(std::shared_ptr<const Vector<D>> b)
	{
		auto p = std::dynamic_pointer_cast<const HipVector<D>>(b);
		if (!p) throw 3; // same failure mode as SchurHelper.h:129 on a foreign vector type
		return p->v;
	}
	LocalData<D> view(int patch, bool wb) const
	{
		if (patch < 0 || patch >= this->num_local_patches) throw 3;
		std::shared_ptr<HipLDM> ldm(new HipLDM(mirror, patch, wb));
		std::array<int, D>      lengths, strides;
		int                     s = 1;
		for (size_t i = 0; i < D; i++) {
			lengths[i] = ctx->n;
			strides[i] = s;
			s *= ctx->n;
		}
		return LocalData<D>(ldm->data, strides, lengths, ldm);
	}
	LocalData<D>       getLocalData(int p) override { return view(p, true); }
	const LocalData<D> getLocalData(int p) const override { return view(p, false); }
	void set(double a) override { check(te_vec_set(v, a)); }
	void scale(double a) override { check(te_vec_scale(v, a)); }
	void shift(double d) override { check(te_vec_shift(v, d)); }
	void copy(std::shared_ptr<const Vector<D>> b) override { check(te_vec_copy(v, raw(b))); }
	void add(std::shared_ptr<const Vector<D>> b) override { check(te_vec_add(v, raw(b))); }
	void addScaled(double a, std::shared_ptr<const Vector<D>> b) override { check(te_vec_add_scaled(v, a, raw(b))); }
	void addScaled(double alpha, std::shared_ptr<const Vector<D>> a, double beta, std::shared_ptr<const Vector<D>> b) override
	{
		check(te_vec_add_scaled2(v, alpha, raw(a), beta, raw(b)));
	}
	void scaleThenAdd(double a, std::shared_ptr<const Vector<D>> b) override { check(te_vec_scale_then_add(v, a, raw(b))); }
	void scaleThenAddScaled(double a, double be, std::shared_ptr<const Vector<D>> b) override
	{
		check(te_vec_scale_then_add_scaled(v, a, be, raw(b)));
	}
	void scaleThenAddScaled(double a, double be, std::shared_ptr<const Vector<D>> b, double ga,
	                        std::shared_ptr<const Vector<D>> c) override
	{
		check(te_vec_scale_then_add_scaled2(v, a, be, raw(b), ga, raw(c)));
	}
	// local partial results + the reference's own MPI_Allreduce (Vector.h:294,306,319)
	double twoNorm() const override
	{
		double s, gs;
		check(te_vec_two_norm_sq(v, &s));
		MPI_Allreduce(&s, &gs, 1, MPI_DOUBLE, MPI_SUM, this->comm);
		return sqrt(gs);
	}
	double infNorm() const override
	{
		double s, gs;
		check(te_vec_inf_norm(v, &s));
		MPI_Allreduce(&s, &gs, 1, MPI_DOUBLE, MPI_MAX, this->comm);
		return gs;
	}
	double dot(std::shared_ptr<const Vector<D>> b) const override
	{
		double s, gs;
		check(te_vec_dot(v, raw(b), &s));
		MPI_Allreduce(&s, &gs, 1, MPI_DOUBLE, MPI_SUM, this->comm);
		return gs;
	}
};

template <size_t D> class HipVG : public VectorGenerator<D>
{
	std::shared_ptr<Context> ctx;
	int                      level;

	public:
	HipVG(std::shared_ptr<Context> ctx_, int level_) : ctx(ctx_), level(level_) {}
	std::shared_ptr<Vector<D>> getNewVector() override { return std::shared_ptr<Vector<D>>(new HipVector<D>(ctx, level)); }
};

template <size_t D> class HipOperator : public Operator<D>
{
	std::shared_ptr<Context> ctx;
	int                      level;

	public:
	HipOperator(std::shared_ptr<Context> ctx_, int level_) : ctx(ctx_), level(level_) {}
	void apply(std::shared_ptr<const Vector<D>> x, std::shared_ptr<Vector<D>> b) const override
	{
		check(te_apply(ctx->g, level, HipVector<D>::raw(x), const_cast<te_vec *>(HipVector<D>::raw(b))));
	}
};

template <size_t D> class HipSmoother : public GMG::Smoother<D>
{
	std::shared_ptr<Context> ctx;
	int                      level, kind;
	double                   omega;

	public:
	/// kind: TE_SMOOTH_PATCH_SOLVE (the reference's FFTBlockJacobiSmoother), TE_SMOOTH_JACOBI, TE_SMOOTH_RBGS, or (D = 2)
	/// TE_SMOOTH_PATCH_BCGS: the block-Jacobi sweep over BiCGStabSolver<2>(p_operator, ps_tol, ps_max_it) that
	/// apps/2d/steady.cpp:326-327 builds for --patch_solver bcgs; its stopping rule through te_gmg_set_patch_bcgs(ctx->g, ...)
	HipSmoother(std::shared_ptr<Context> ctx_, int level_, int kind_ = TE_SMOOTH_PATCH_SOLVE, double omega_ = 6.0 / 7.0)
	: ctx(ctx_), level(level_), kind(kind_), omega(omega_)
	{
	}
	void smooth(std::shared_ptr<const Vector<D>> f, std::shared_ptr<Vector<D>> u) const override
	{
		check(te_smooth(ctx->g, level, HipVector<D>::raw(f), const_cast<te_vec *>(HipVector<D>::raw(u)), kind, omega, 1));
	}
};

template <size_t D> class HipRestrictor : public GMG::Restrictor<D>
{
	std::shared_ptr<Context> ctx;
	int                      fine_level;

	public:
	HipRestrictor(std::shared_ptr<Context> ctx_, int fine_level_) : ctx(ctx_), fine_level(fine_level_) {}
	void restrict(std::shared_ptr<Vector<D>> coarse, std::shared_ptr<const Vector<D>> fine) const override
	{
		check(te_restrict(ctx->g, fine_level, HipVector<D>::raw(fine), const_cast<te_vec *>(HipVector<D>::raw(coarse))));
	}
};

template <size_t D> class HipInterpolator : public GMG::Interpolator<D>
{
	std::shared_ptr<Context> ctx;
	int                      fine_level;

	public:
	HipInterpolator(std::shared_ptr<Context> ctx_, int fine_level_) : ctx(ctx_), fine_level(fine_level_) {}
	void interpolate(std::shared_ptr<const Vector<D>> coarse, std::shared_ptr<Vector<D>> fine) const override
	{
		check(te_prolong_add(ctx->g, fine_level, HipVector<D>::raw(coarse), const_cast<te_vec *>(HipVector<D>::raw(fine))));
	}
};

/// The tri-/bilinear interpolator (TE_INTERP_LINEAR, include/te_hip.h): what GMG/TriLinIntp.h was written for, patch-local plus
/// face ghosts. Single rank: on a sharded hierarchy interpolate() throws (TE_ESTATE).
template <size_t D> class HipLinearInterpolator : public GMG::Interpolator<D>
{
	std::shared_ptr<Context> ctx;
	int                      fine_level;

	public:
	HipLinearInterpolator(std::shared_ptr<Context> ctx_, int fine_level_) : ctx(ctx_), fine_level(fine_level_) {}
	void interpolate(std::shared_ptr<const Vector<D>> coarse, std::shared_ptr<Vector<D>> fine) const override
	{
		check(te_prolong_linear_add(ctx->g, fine_level, HipVector<D>::raw(coarse), const_cast<te_vec *>(HipVector<D>::raw(fine))));
	}
};

/// The whole preconditioner M = GMG cycle in one native call (what CycleFactory3d::getCycle returns). It prolongs with the
/// solver's interpolator (te_gmg_set_interpolator; TE_INTERP_DIRECT unless set): the second constructor sets it first.
template <size_t D> class HipCycle : public Operator<D>
{
	std::shared_ptr<Context> ctx;
	te_cycle_opts            opts;

	public:
	HipCycle(std::shared_ptr<Context> ctx_, const te_cycle_opts &o) : ctx(ctx_), opts(o) {}
	HipCycle(std::shared_ptr<Context> ctx_, const te_cycle_opts &o, int interpolator) : ctx(ctx_), opts(o)
	{
		check(te_gmg_set_interpolator(ctx->g, interpolator));
	}
	int interpolator() const { return te_gmg_interpolator(ctx->g); }
	void apply(std::shared_ptr<const Vector<D>> f, std::shared_ptr<Vector<D>> u) const override
	{
		check(te_vcycle(ctx->g, &opts, HipVector<D>::raw(f), const_cast<te_vec *>(HipVector<D>::raw(u))));
	}
};
// ------------------------------------------------------------------------- Schur-complement route (single rank)
template <size_t D> class HipSchurVG : public VectorGenerator<D - 1>
{
	std::shared_ptr<Context> ctx;
	int                      level;

	public:
	HipSchurVG(std::shared_ptr<Context> ctx_, int level_ = 0) : ctx(ctx_), level(level_) {}
	std::shared_ptr<Vector<D - 1>> getNewVector() override
	{
		return std::shared_ptr<Vector<D - 1>>(new HipVector<D - 1>(ctx, level, true));
	}
};

/// The Schur system S gamma = g of the reference's --schur drivers, solved by the reference's own BiCGStab<D-1>:
///   auto vg = make_shared<HipSchurVG<3>>(ctx); auto S = make_shared<HipSchurOp<3>>(ctx);
///   auto gamma = vg->getNewVector(), g = vg->getNewVector(); S->rhs(f, g);
///   BiCGStab<2>::solve(vg, S, gamma, g, make_shared<HipChebPrec<3>>(ctx)); S->solution(f, gamma, u);
template <size_t D> class HipSchurOp : public Operator<D - 1>
{
	std::shared_ptr<Context> ctx;
	int                      level;

	public:
	HipSchurOp(std::shared_ptr<Context> ctx_, int level_ = 0) : ctx(ctx_), level(level_) {}
	void apply(std::shared_ptr<const Vector<D - 1>> x, std::shared_ptr<Vector<D - 1>> b) const override
	{
		check(te_schur_apply(ctx->g, level, HipVector<D - 1>::raw(x), const_cast<te_vec *>(HipVector<D - 1>::raw(b))));
	}
	/// g = Interp(Solve(f, 0)): the right-hand side (solveWithInterface's diff at gamma = 0, SchurHelper.h:280-297)
	void rhs(std::shared_ptr<const Vector<D>> f, std::shared_ptr<Vector<D - 1>> g) const
	{
		HipVector<D>     u(ctx, level);
		HipVector<D - 1> zero(ctx, level, true);
		check(te_solve_with_interface(ctx->g, level, HipVector<D>::raw(f), u.v, zero.v, const_cast<te_vec *>(HipVector<D - 1>::raw(g))));
	}
	/// u = Solve(f, gamma): the domain solution once gamma solves the Schur system
	void solution(std::shared_ptr<const Vector<D>> f, std::shared_ptr<const Vector<D - 1>> gamma, std::shared_ptr<Vector<D>> u) const
	{
		check(te_solve_with_interface(ctx->g, level, HipVector<D>::raw(f), const_cast<te_vec *>(HipVector<D>::raw(u)),
		                              HipVector<D - 1>::raw(gamma), nullptr));
	}
};

template <size_t D> class HipChebPrec : public Operator<D - 1>
{
	std::shared_ptr<Context> ctx;
	int                      level;

	public:
	HipChebPrec(std::shared_ptr<Context> ctx_, int level_ = 0) : ctx(ctx_), level(level_) {}
	void apply(std::shared_ptr<const Vector<D - 1>> x, std::shared_ptr<Vector<D - 1>> b) const override
	{
		check(te_schur_cheb(ctx->g, level, HipVector<D - 1>::raw(x), const_cast<te_vec *>(HipVector<D - 1>::raw(b))));
	}
};
// ------------------------------------------------------------------------- MAC gradient, divergence, projection
/// A face vector of one level (te_vec_create_faces): per local patch D n^D + D n^(D-1) doubles -- the blocks LO_0 .. LO_{D-1}
/// (n^D each, cell layout: the component on the lower a-face of the cell), then HI_0 .. HI_{D-1} (n^(D-1) each: the patch's upper
/// a-face). Not a Vector<D>: the reference has no face-centred vector. Every te_vec_* BLAS-1 call takes raw().
template <size_t D> class HipFaceVector
{
	public:
	std::shared_ptr<Context> ctx;
	te_vec                  *v = nullptr;
	int                      level;
	HipFaceVector(std::shared_ptr<Context> ctx_, int level_ = 0) : ctx(ctx_), level(level_) { check(te_vec_create_faces(ctx->g, level, &v)); }
	~HipFaceVector() { te_vec_destroy(v); }
	HipFaceVector(const HipFaceVector &) = delete;
	HipFaceVector &operator=(const HipFaceVector &) = delete;
	te_vec        *raw() const { return v; }
	/// values on one face of a patch, n^(D-1)
	size_t faceSize() const
	{
		size_t nf = 1;
		for (size_t i = 1; i < D; i++) nf *= ctx->n;
		return nf;
	}
	/// doubles per patch
	size_t patchSize() const { return D * faceSize() * ctx->n + D * faceSize(); }
	int    numLocalPatches() const { return (int) (te_vec_size(v) / patchSize()); }
	/// where block LO_a / HI_a starts inside a patch's run of doubles
	size_t loOffset(int a) const { return (size_t) a * faceSize() * ctx->n; }
	size_t hiOffset(int a) const { return D * faceSize() * ctx->n + (size_t) a * faceSize(); }
	void upload(int first_patch, int npatches, const double *host) { check(te_vec_upload_patches(v, first_patch, npatches, host)); }
	void download(int first_patch, int npatches, double *host) const { check(te_vec_download_patches(v, first_patch, npatches, host)); }
};

/// G = grad u with the ghosts te_apply uses; bdata: a boundary vector (te_vec_create_boundary) or NULL. Collective.
template <size_t D> void gradient(std::shared_ptr<const Vector<D>> u, HipFaceVector<D> &G, const te_vec *bdata = nullptr)
{
	check(te_gradient(G.ctx->g, G.level, HipVector<D>::raw(u), bdata, G.raw()));
}
/// out = alpha div U (patch-local)
template <size_t D> void divergence(const HipFaceVector<D> &U, std::shared_ptr<Vector<D>> out, double alpha = 1.0)
{
	check(te_divergence(U.ctx->g, U.level, alpha, U.raw(), const_cast<te_vec *>(HipVector<D>::raw(out))));
}
/// U -= alpha grad p in one pass. Collective.
template <size_t D> void project(HipFaceVector<D> &U, std::shared_ptr<const Vector<D>> p, double alpha = 1.0, const te_vec *bdata = nullptr)
{
	check(te_project(U.ctx->g, U.level, alpha, HipVector<D>::raw(p), bdata, U.raw()));
}
} // namespace tehip
#endif
