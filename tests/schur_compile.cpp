// Compile-only check (where the reference tree is present): the Schur-route adaptors are real subclasses of the reference's
// plugin interfaces over Vector<D-1>, and the reference's own BiCGStab<D-1> instantiates against them -- the --schur
// [--prec cheb] block of apps/3d/steady.cpp:336-420 and apps/2d/steady.cpp:383-480 on the native path. Nothing runs here.
#include <Thunderegg/BiCGStab.h>
#include <HipGMG.h>

template <size_t D> int schurSolve(const te_hier *h, bool cheb)
{
	using namespace tehip;
	std::shared_ptr<Context>                ctx(new Context(h));
	std::shared_ptr<VectorGenerator<D>>     vg(new HipVG<D>(ctx, 0));
	std::shared_ptr<VectorGenerator<D - 1>> svg(new HipSchurVG<D>(ctx, 0));
	std::shared_ptr<HipSchurOp<D>>          S(new HipSchurOp<D>(ctx, 0));
	std::shared_ptr<Operator<D - 1>>        M;
	if (cheb) M.reset(new HipChebPrec<D>(ctx, 0));
	auto f = vg->getNewVector(), u = vg->getNewVector();
	auto gamma = svg->getNewVector(), g = svg->getNewVector();
	S->rhs(f, g);
	int its = BiCGStab<D - 1>::solve(svg, S, gamma, g, M); // the drivers' call, unchanged
	S->solution(f, gamma, u);
	return its;
}

int drive3d(const te_hier *h) { return schurSolve<3>(h, true); }
int drive2d(const te_hier *h) { return schurSolve<2>(h, true); }
