// CPU, syntax only: one projection step of a flow solver written against the reference's Vector<D> interface -- divergence of a
// face vector, boundary fold, (solve elsewhere), projection -- through tehip::HipFaceVector / gradient / divergence / project
// (thunderegg/HipGMG.h). Compiled by tests/test_projection_host.py against the reference's own headers; nothing is run.
#include <HipGMG.h>

template <size_t D> void projectionStep(std::shared_ptr<tehip::Context> ctx, double dt, const te_vec *bdata, std::vector<double> &host)
{
	tehip::HipFaceVector<D>    U(ctx, 0), G(ctx, 0);
	std::shared_ptr<Vector<D>> f(new tehip::HipVector<D>(ctx, 0)), p(new tehip::HipVector<D>(ctx, 0));
	host.resize(U.patchSize() * U.numLocalPatches());
	U.upload(0, U.numLocalPatches(), host.data());
	tehip::divergence<D>(U, f, 1.0 / dt);
	tehip::check(te_add_boundary_rhs(ctx->g, 0, bdata, const_cast<te_vec *>(tehip::HipVector<D>::raw(f))));
	tehip::gradient<D>(p, G, bdata);
	tehip::project<D>(U, p, dt, bdata);
	tehip::check(te_vec_add_scaled(G.raw(), -1.0, U.raw()));
	U.download(0, U.numLocalPatches(), host.data());
	if (U.hiOffset(0) != D * U.loOffset(1)) throw 3;
}
template void projectionStep<3>(std::shared_ptr<tehip::Context>, double, const te_vec *, std::vector<double> &);
template void projectionStep<2>(std::shared_ptr<tehip::Context>, double, const te_vec *, std::vector<double> &);
