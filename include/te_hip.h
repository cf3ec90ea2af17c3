/* te_hip.h — C ABI of the MI355X-native GMG V-cycle path (libte_hip.so).
 *
 * Drop-in boundary for GEM3D/pressurePoissonSolver's src/Thunderegg GMG hot path. Every entry
 * point names the reference interface it stands behind (paths relative to the reference
 * root). Plain pointers, sizes and opaque handles only; no C++ or torch types. All functions
 * return TE_OK (0) or a negative TE_E* code; te_last_error() gives the message. The C++
 * adaptors in pressurepoissonsolver_amd/thunderegg/ turn a non-zero status into the
 * reference's own error convention (`throw 3;`, e.g. GMG/InterLevelComm.h:175).
 *
 * Vector layout on the host side of upload/download is the reference's: patch-major, x-fastest,
 * interior cells only, patch p at offset p*n^dim (src/Thunderegg/PetscVector.h:70-98), with
 * patches in THIS library's local order (te_hier_level_ids gives the tree node id of each).
 */
#ifndef TE_HIP_H
#define TE_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define TE_OK 0
#define TE_EINVAL -1   /* bad argument / shape mismatch */
#define TE_EHIP -2     /* HIP runtime error (no device, launch failure, OOM) */
#define TE_ESTATE -3   /* call not valid in the object's current state */
#define TE_EIO -4      /* mesh file unreadable */
#define TE_EUNSUPPORTED -5
#define TE_ENOMEM -6    /* host allocation failed */

typedef struct te_mesh te_mesh; /* octree / quadtree              (OctTree.h:34 Tree<D>) */
typedef struct te_hier te_hier; /* host level tables, one rank    (ThundereggDomGen.h:95-222 + Domain.h) */
typedef struct te_gmg  te_gmg;  /* device-resident level stack    (GMG/CycleFactory3d.cpp:69-134 product) */
typedef struct te_vec  te_vec;  /* device vector on one level     (Vector.h:179 Vector<D>, PetscVector.h:59) */

const char *te_last_error(void);
const char *te_version(void);

/* ---------------------------------------------------------------- mesh (host only, no GPU) */
/* Tree<D>::Tree(std::string) OctTree.h:90-118 */
int te_mesh_read(const char *path, int dim, te_mesh **out);
/* one root node on the unit box (what a 1-node mesh file such as apps/3d/meshes/1uni.bin holds) */
int te_mesh_unit_root(int dim, te_mesh **out);
/* Tree<D>::refineLeaves OctTree.h:119-179 (== one unit of the drivers' --divide) */
int te_mesh_refine_leaves(te_mesh *m);
int te_mesh_num_nodes(const te_mesh *m);
int te_mesh_num_levels(const te_mesh *m);
int te_mesh_dim(const te_mesh *m);
/* node table in ascending id order; any pointer may be NULL.
 * ilp[N][3] = id, level, parent; lengths/starts [N][dim]; nbr [N][2*dim]; child [N][2^dim] */
int  te_mesh_get_nodes(const te_mesh *m, int32_t *ilp, double *lengths, double *starts,
                       int32_t *nbr, int32_t *child);
/* The leaves (nodes without children): their number, and their ids in ascending order (ids[te_mesh_num_leaves]). Level 0 of every
 * hierarchy built from the mesh holds exactly these nodes. */
int te_mesh_num_leaves(const te_mesh *m);
int te_mesh_leaves(const te_mesh *m, int32_t *ids);
/* 1: the tree is FACE-balanced -- two leaves that share a face differ by at most one level (faces are all the solver reads; edges
 * and corners are not looked at); 0: it is not; < 0: error. The reference never checks (its mesh files are balanced by whoever wrote
 * them). */
int te_mesh_is_balanced(const te_mesh *m);
/* Adaptive regridding: *out = a NEW tree made from `m` (untouched) and one flag per named leaf, flags[i] for leaf ids[i]: +1 refine,
 * 0 keep, -1 coarsen; leaves not named count as 0. TE_EINVAL for an unknown id, a node that is not a leaf, an id named twice or any
 * other flag value. The reference has Tree::refineNode (OctTree.h:180) and nothing else: no balance, no coarsening. The rule:
 *   1. Refinement set R. Start with the leaves flagged +1. Repeat until nothing changes: for every X in R and every side s such that
 *      X has no same-level neighbour on s, s is an outer side of X's orthant in its parent, and X's parent has a neighbour Y on s that
 *      is a leaf: add Y to R (a flag of -1 on Y loses). With a balanced `m` every leaf is refined at most once and *out is balanced;
 *      with an unbalanced `m` *out may be unbalanced -- nothing is repaired.
 *   2. Coarsening. A node P is coarsened when all 2^dim children of P are leaves, all of them are flagged -1, none of them is in R,
 *      and for every side s of P the same-level neighbour Q = nbr[s] of P is absent, or a leaf that is not in R, or split with each of
 *      Q's children on side s^1 a leaf that is not in R. Every family is judged against the state after step 1, not against the
 *      other families: two adjacent families may both go.
 *   3. Apply. R is refined in ascending (depth, id) order, each node as Tree::refineNode does it, so the new ids are ++max_id in that
 *      order and then orthant order (max_id = the largest id of `m`). Then the accepted families are removed in ascending parent id:
 *      the children are erased, P becomes a leaf, and the erased ids are cleared from their neighbours' nbr[]. num_levels is
 *      recomputed. Surviving nodes keep their ids, so ids may have gaps afterwards (te_mesh_get_nodes lists rows in ascending id).
 * Flagging every leaf +1 gives, node for node and id for id, what te_mesh_refine_leaves gives. A leaf changes by at most one level
 * per call. */
int te_mesh_adapt(const te_mesh *m, int count, const int32_t *ids, const int32_t *flags, te_mesh **out);
void te_mesh_destroy(te_mesh *m);

/* ----------------------------------------------------- level hierarchy (host only, no GPU) */
/* ThundereggDomGen<D>(t, ns, neumann) + the level loop of CycleFactory3d::getCycle
 * (CycleFactory3d.cpp:98-127; max_levels / patches_per_proc from GMG/CycleOpts.h:55-63).
 * The Zoltan partition is replaced by contiguous Morton ranges over `nranks`. */
int te_hier_build(const te_mesh *m, int n, int neumann, int max_levels, double patches_per_proc,
                  int rank, int nranks, te_hier **out);
/* The same with the placement of the small levels over the ranks spelled out instead of taken from the environment
 * (te_hier_build reads TE_AGGLOMERATE, TE_AGGLOMERATE_MAX, TE_REPLICATE once per call and comes here): a level with fewer
 * than `agglomerate` patches per rank and at most `agglomerate_max` patches in total, and every level below it, is gathered --
 * on every rank (`replicate` != 0; 3D, and since round 5 2D) or on rank 0. A negative value = the default (64, 64, 1); agglomerate = 0 never
 * gathers. What the reference does instead is cut the hierarchy (patches_per_proc, CycleFactory3d.cpp:104). Every rank must
 * pass the same values: te_vcycle / te_bicgstab compare them across the ranks before the first cycle (TE_ESTATE, by name). */
int te_hier_build_placed(const te_mesh *m, int n, int neumann, int max_levels, double patches_per_proc,
                         int rank, int nranks, double agglomerate, int agglomerate_max, int replicate, te_hier **out);
/* te_hier_build_placed with one boundary kind per SIDE OF THE DOMAIN: bit s of `neumann_sides` set = side s is a Neumann boundary,
 * clear = Dirichlet; s = 2 * axis + upper (west, east, south, north, bottom, top: Side.h:51-56, the numbering of face tables
 * everywhere here). The reference's drivers have one --neumann flag for all sides (apps/3d/steady.cpp:318-334) although its
 * patch operator takes one flag per side (PatchInfo.h neumann bitset, StarPatchOp.h:39-65): this is the call for walls and inflow
 * (Neumann) next to an outflow or a free surface (Dirichlet). `neumann` != 0 of the two calls above = every bit set.
 * TE_EINVAL for a bit at or above 2 * dim. Every rank must pass the same mask (compared with the placement, TE_ESTATE by name).
 * One kind per side of the domain, not per patch face; no Robin conditions. */
int te_hier_build_bc(const te_mesh *m, int n, int neumann_sides, int max_levels, double patches_per_proc,
                     int rank, int nranks, double agglomerate, int agglomerate_max, int replicate, te_hier **out);
/* the mask ((1 << 2 dim) - 1 for a hierarchy built with neumann = 1, 0 with neumann = 0) */
int te_hier_neumann_sides(const te_hier *h);
/* 1: every side is Neumann -- the operator has the constant null space, and the driver subtracts the mean of f with te_integrate /
 * te_volume (apps/3d/steady.cpp:330-334); 0: the system is regular, no mean subtraction. */
int te_hier_singular(const te_hier *h);
/* The physical faces (no neighbour) of this rank's patches of a level, numbered in (patch, side) order: the blocks of a boundary
 * vector (te_vec_create_boundary). bface_index[P_local][2*dim] = the face's number, -1 on a face with a neighbour. Sharded
 * hierarchies number their local faces; on a level that lives on every rank, every rank numbers the whole level. Replaces nothing
 * in the reference (Init.cpp walks PatchInfo::hasNbr per patch). */
int te_hier_num_bfaces(const te_hier *h, int level, int *num_bfaces);
int te_hier_bface_index(const te_hier *h, int level, int32_t *bface_index);
/* the placement this hierarchy was built with (any pointer may be NULL) */
int te_hier_placement(const te_hier *h, double *agglomerate, int *agglomerate_max, int *replicate);
int te_hier_num_levels(const te_hier *h);
int te_hier_dim(const te_hier *h);
int te_hier_n(const te_hier *h);
/* level 0 = finest. P_local = this rank's patches, P_global = all ranks'. */
int te_hier_level_sizes(const te_hier *h, int level, int *P_local, int *P_global);
/* 1: the level lives on EVERY rank (a gathered coarse level, TE_REPLICATE: each rank holds and computes all
 * of it, P_local == P_global, and the `rank` column of te_hier_level_tables names the calling rank for every patch); 0: every
 * patch has one owner; < 0: error. Replaces nothing in the reference (CycleFactory3d.cpp:104 cuts the hierarchy instead). */
int te_hier_level_replicated(const te_hier *h, int level);
/* Global tables of one level (Morton order); any pointer may be NULL.
 * id[P] rank[P] local[P] starts[P][dim] lengths[P][dim] nbr_kind[P][2dim] (0 none, 1 normal,
 * 2 coarse, 3 fine) nbr[P][2dim][4] nbr_orth[P][2dim] parent[P] orth_on_parent[P] */
int te_hier_level_tables(const te_hier *h, int level, int32_t *id, int32_t *rank, int32_t *local,
                         double *starts, double *lengths, int32_t *nbr_kind, int32_t *nbr,
                         int32_t *nbr_orth, int32_t *parent, int32_t *orth_on_parent);
/* local -> global patch index of this rank's patches */
int  te_hier_level_l2g(const te_hier *h, int level, int32_t *l2g);
/* Where the patches of level 0 (= the leaves of the mesh) sit in the TREE, global order, P_global entries each: id = the tree node
 * id, tree_parent = the id of its parent in the tree (-1: the root), orthant = its orthant there (-1: the root). Not the `parent`
 * column of te_hier_level_tables, which names a patch of the next coarser LEVEL. Any pointer may be NULL. What te_vec_regrid matches
 * two meshes by; replaces nothing in the reference (it never moves a solution between meshes). */
int  te_hier_leaf_tree(const te_hier *h, int32_t *id, int32_t *tree_parent, int32_t *orthant);
/* The interfaces of a level, the unknowns of the Schur-complement route: SchurHelper<D>::indexDomainIfacesLocal
 * (SchurHelper.h:377-397), the first-seen order of SchurInfo<D>::getIds() over the patches in this library's order.
 * iface_index[P][2*dim] = the interface patch p sees on side s, -1 on a physical face. Single-rank hierarchies only
 * (TE_ESTATE on a sharded one). */
int  te_hier_num_ifaces(const te_hier *h, int level, int *num_ifaces);
int  te_hier_iface_index(const te_hier *h, int level, int32_t *iface_index);
void te_hier_destroy(te_hier *h);

/* ------------------------------------------------------------------------ device objects */
typedef struct {
	int32_t pre_sweeps, post_sweeps, coarse_sweeps, mid_sweeps; /* GMG/CycleOpts.h:64-79 */
	int32_t cycle_type; /* 0 "V" (VCycle.h), 1 "W" (WCycle.h) */
	int32_t smoother;   /* TE_SMOOTH_* */
	double  omega;      /* Jacobi weight */
	int32_t exact_coarse; /* pointwise smoothers: exact patch solve on a 1-patch coarsest level */
	int32_t fuse;         /* 0: one kernel per reference call (apply, scaleThenAdd, restrict, set, ...);
	                         1: inside te_vcycle use the fused kernels whose results are BIT-IDENTICAL to 0
	                            (residual+restrict, zero-guess first sweep, sweep on u + P e);
	                         2: additionally to 1, with one RB-GS pre-sweep on a uniformly refined 3D level,
	                            the sweep from the zero iterate, the residual and its restriction are one pass over f;
	                            the coarse right-hand side differs from 1 by a few ulp along patch faces (the ghost
	                            term of the residual is added separately), independent of the partition; with one
	                            block-Jacobi pre-sweep the residual after the exact patch solves is taken on the face
	                            layers only (it vanishes inside a patch up to the rounding of the solve);
	                         3 (default): 2, and with exactly one RB-GS pre-sweep and a post-sweep in a V-cycle the
	                            iterate between them is never stored: the post-sweep kernel recomputes it from f
	                            (bit-identical to 2).
	                         In 2 and 3 the fused pre-sweep forms the residual it restricts on RED cells only and takes
	                         the black cells' residual as exactly 0: a black cell was relaxed last, from the very values
	                         its residual is formed with, so what is dropped is the rounding of that one update (~1e-16
	                         relative in the coarse right-hand side) -- inside every stated tolerance, but not
	                         bit-identical to 1 */
} te_cycle_opts;

#define TE_SMOOTH_PATCH_SOLVE 0 /* reference: FFTBlockJacobiSmoother.h:55-58 (block Jacobi, exact patch solves) */
#define TE_SMOOTH_JACOBI 1      /* weighted point Jacobi */
#define TE_SMOOTH_RBGS 2        /* patch-local red-black Gauss-Seidel, neighbour ghosts frozen */
#define TE_SMOOTH_PATCH_BCGS 3  /* 2D only: block Jacobi whose patch solves are the reference's OTHER patch solver, PatchSolvers/
                                   BiCGStabSolver.h:114-132 (apps/2d/steady.cpp:326-327, --patch_solver bcgs): per patch, unpreconditioned
                                   BiCGStab<2>::solve (BiCGStab.h:45-106) on StarPatchOp<2>::apply from the patch's current values, to
                                   te_gmg_set_patch_bcgs's tolerance; one workgroup per patch, the Krylov vectors in registers */

void te_cycle_opts_default(te_cycle_opts *o);

/* Creates the HIP stream, uploads every level's tables, allocates all scratch. Fails with
 * TE_EHIP when no gfx950 device is usable — there is no CPU fallback.
 * device < 0 selects the current device. */
int  te_gmg_create(const te_hier *h, int device, te_gmg **out);
void te_gmg_destroy(te_gmg *g);
int  te_gmg_num_levels(const te_gmg *g);
int  te_gmg_sync(te_gmg *g);            /* hipStreamSynchronize on the solver stream */
void *te_gmg_stream(te_gmg *g);         /* hipStream_t, for event timing by the caller */

/* VectorGenerator<D>::getNewVector (Vector.h:323-327; DomainVG Domain.h:415-429): zero-filled */
int    te_vec_create(te_gmg *g, int level, te_vec **out);
/* SchurHelper<D>::getNewSchurVec (SchurHelper.h:156-160): an interface vector of `level`, num_ifaces * n^(dim-1) doubles,
 * one block per interface (te_hier_num_ifaces), zero-filled. Every te_vec_* call takes it (te_vec_upload_patches /
 * te_vec_download_patches count interface blocks instead of patches); the domain operators (te_apply, te_smooth, te_vcycle,
 * te_bicgstab, ...) refuse it with TE_EINVAL. Single rank: TE_ESTATE on a sharded hierarchy. */
int    te_vec_create_iface(te_gmg *g, int level, te_vec **out);
/* A boundary vector of `level`: te_hier_num_bfaces * n^(dim-1) doubles, one block per physical face of this rank's patches in
 * te_hier_bface_index order, a block laid out like an interface block (the face's remaining axes, x fastest), zero-filled. The
 * boundary values g (Dirichlet faces) or the derivative along the face's axis g_n (Neumann faces) of a driver whose boundary
 * data is not one of the canned problems' or changes every time step. Every te_vec_* call takes it (te_vec_upload_patches /
 * te_vec_download_patches count blocks); the domain operators refuse it with TE_EINVAL. Exists on sharded hierarchies too.
 * Replaces nothing in the reference (its boundary data are std::function callbacks evaluated inside Init.cpp's loops). */
int    te_vec_create_boundary(te_gmg *g, int level, te_vec **out);
/* A face vector of `level`: one component per cell face, ALONG THE AXIS (not the outward normal), stored per local patch -- a face
 * shared by two patches is stored by both. Per patch, D = dim, n = cells per axis, D n^D + D n^(D-1) doubles in this order:
 * blocks LO_a, a = 0..D-1, n^D doubles each in the cell layout of a domain vector (x fastest): the component on the LOWER a-face
 * of the cell; then blocks HI_a, a = 0..D-1, n^(D-1) doubles each, laid out like an interface / boundary block of side 2a+1: the
 * component on the patch's UPPER a-face. Zero-filled. Every te_vec_* call takes it (te_vec_upload_patches / _download_patches
 * count patches); the domain operators refuse it with TE_EINVAL; te_gradient, te_divergence and te_project refuse anything else
 * in its place. Exists on sharded hierarchies (local patches) and on every level. Replaces nothing in the reference. */
int    te_vec_create_faces(te_gmg *g, int level, te_vec **out);
void   te_vec_destroy(te_vec *v);
size_t te_vec_size(const te_vec *v);                 /* doubles (local patches * n^dim) */
int    te_vec_upload(te_vec *v, const double *host); /* Vector<D>::getLocalData write path */
int    te_vec_download(const te_vec *v, double *host);
/* Vector<D>::getLocalData(i) (Vector.h:214-215, PetscVector.h:87-98) for patches [first_patch, first_patch+npatches):
 * host holds npatches * n^dim doubles in the same layout. The per-patch data plane of the C++ adaptor
 * (HipVector::getLocalData) and of Init-style fill loops (apps/shared/Init.cpp:152-245). */
int    te_vec_upload_patches(te_vec *v, int first_patch, int npatches, const double *host);
int    te_vec_download_patches(const te_vec *v, int first_patch, int npatches, double *host);
void  *te_vec_device_ptr(te_vec *v);

/* Vector<D> BLAS-1 virtuals, Vector.h:190-321 (same names, same argument order) */
int te_vec_set(te_vec *v, double alpha);
int te_vec_scale(te_vec *v, double alpha);
int te_vec_shift(te_vec *v, double delta);
int te_vec_copy(te_vec *v, const te_vec *b);
int te_vec_add(te_vec *v, const te_vec *b);
int te_vec_add_scaled(te_vec *v, double alpha, const te_vec *b);
int te_vec_add_scaled2(te_vec *v, double alpha, const te_vec *a, double beta, const te_vec *b);
int te_vec_scale_then_add(te_vec *v, double alpha, const te_vec *b);
int te_vec_scale_then_add_scaled(te_vec *v, double alpha, double beta, const te_vec *b);
int te_vec_scale_then_add_scaled2(te_vec *v, double alpha, double beta, const te_vec *b,
                                  double gamma, const te_vec *c);
/* v[i] *= b[i], for vectors of any one kind (domain, interface, boundary, face); TE_EINVAL when v and b differ in solver, level or
 * kind. Nothing in Vector.h; what beta (.) grad p is for a face vector. */
int te_vec_multiply(te_vec *v, const te_vec *b);
/* local (this rank's) partial results; the caller all-reduces (Vector.h:294,306,319) */
int te_vec_two_norm_sq(const te_vec *v, double *out);
int te_vec_inf_norm(const te_vec *v, double *out);
int te_vec_dot(const te_vec *v, const te_vec *b, double *out);
/* This rank's part of the vector's CHECKSUM: the sum modulo 2^64 of the 64-bit patterns of its values. Integer addition
 * commutes, so the sum of the ranks' parts (modulo 2^64; the caller adds them, as for the norms) does not depend on the order of
 * the patches nor on how they are cut over ranks: a sharded run that is bit-identical to the single-rank run -- what every
 * operation of a cycle is by construction -- prints the same number. How a job on hardware nobody can inspect shows that N
 * ranks computed the very bits one rank computes (bench.py: u_checksum_after_timed_region). A level that lives on every rank
 * counts once (rank 0's), as in te_vec_dot. Replaces nothing in the reference; the equality it proves is the one between
 * `mpirun -np N` and `-np 1` of SchurHelper.h:123-150 / GMG/InterLevelComm.h:169-189 for order-independent operations. */
int te_vec_checksum(const te_vec *v, uint64_t *out);

/* Operator<D>::apply (Operators/Operator.h:37) as SchurDomainOp / DomainWrapOp implement it:
 * f = A u through SchurHelper::apply (SchurHelper.h:360-376) */
int te_apply(te_gmg *g, int level, const te_vec *u, te_vec *f);
/* PatchOperator<D>::apply without interface values, StarPatchOp.h:204-319 (SevenPtPatchOperator.cpp:247-409,
 * FivePtPatchOperator.h:172-261): f = A_patch u per patch, faces with a neighbour closed as homogeneous
 * Dirichlet. The operator the exact patch solves invert; the reference uses it in PatchSolvers/BiCGStabSolver.h:82-85. */
int te_patch_apply(te_gmg *g, int level, const te_vec *u, te_vec *f);
/* r = f - A u  (Cycle.h:60-61 fused: apply + scaleThenAdd(-1, f)) */
int te_residual(te_gmg *g, int level, const te_vec *u, const te_vec *f, te_vec *r);
/* the same with ||r||^2 (this rank's part; Vector.h:294 twoNorm before its MPI_Allreduce and sqrt) summed by the residual
 * kernel itself while r is in registers: per thread in plane order, then wave shuffles -> LDS -> one partial per workgroup
 * -> a fixed-order final pass. No second pass over r (3D and 2D). */
int te_residual_norm_sq(te_gmg *g, int level, const te_vec *u, const te_vec *f, te_vec *r, double *norm_sq);
/* GMG::Smoother<D>::smooth(f, u) (GMG/Smoother.h:39), `sweeps` times */
int te_smooth(te_gmg *g, int level, const te_vec *f, te_vec *u, int smoother, double omega,
              int sweeps);
/* GMG::Restrictor<D>::restrict(coarse, fine) (GMG/Restrictor.h:39) == AvgRstr.h:78-113.
 * `fine_level` is the level of `fine`; coarse lives on fine_level+1. */
int te_restrict(te_gmg *g, int fine_level, const te_vec *fine, te_vec *coarse);
/* GMG::Interpolator<D>::interpolate(coarse, fine) (GMG/Interpolator.h:39) == DrctIntp.h:80-113 */
int te_prolong_add(te_gmg *g, int fine_level, const te_vec *coarse, te_vec *fine);
/* The interpolator of a cycle. DIRECT copies the coarse cell's value to its fine cells (order 1); LINEAR is tri-/bilinear (order 2:
 * with AvgRstr the orders add up to more than the operator's 2, and the cycle's convergence factor no longer grows with the depth of
 * the hierarchy). LINEAR stands behind GMG/TriLinIntp.h (which the reference's build leaves out), restated so that it stays
 * patch-local plus face ghosts. E = the coarse patch's values extended to indices -1 .. n per axis: with ONE axis out of range the
 * ghost te_apply's stencil reads there for homogeneous boundary data (the neighbour's cell; 2 gamma - m on a coarse/fine face, gamma
 * the interface value of SchurHelper::interpolateToInterface and m the cell just inside; -m on a physical Dirichlet face, +m on a
 * Neumann face); with k >= 2 axes out of range (patch edges and corners), m = the patch's own cell with those indices clamped, the
 * sum over the out-of-range axes, in ascending order, of the face ghost of m through that axis, minus (k - 1) m -- no edge or corner
 * neighbour is read. Fine cell i of a child in orthant o takes, per axis a, c = (i + o_a n) >> 1 and d = -1 (i even) / +1 (i odd),
 * and v <- 0.75 E[c] + 0.25 E[c + d], x then y then z (27/9/9/9/3/3/3/1 over 64 in 3D, 9/3/3/1 over 16 in 2D); fine += v. A patch
 * that copies through (orthant -1) receives fine += coarse as in DrctIntp. */
#define TE_INTERP_DIRECT 0 /* GMG/DrctIntp.h:80-113 (the default) */
#define TE_INTERP_LINEAR 1 /* stands behind GMG/TriLinIntp.h, restated as above */
/* GMG::Interpolator<D>::interpolate(coarse, fine) with TE_INTERP_LINEAR: the arguments and checks of te_prolong_add. Makes the COARSE
 * level's ghosts current as te_apply does. Single rank: TE_ESTATE on a sharded hierarchy -- the sharded form is future work (the ring
 * of the parent's block for children on another rank, and the proof of bit-identity with the single-rank run, are missing). */
int te_prolong_linear_add(te_gmg *g, int fine_level, const te_vec *coarse, te_vec *fine);
/* Which prolongation te_vcycle, and through it te_bicgstab, uses (te_cycle_opts keeps its layout). With LINEAR the cycle prolongs
 * with te_prolong_linear_add's kernel on the stored iterate and runs plain post-sweeps: every fused form that has DrctIntp's
 * arithmetic in it (the sweeps on u + P e, the unstored iterate of fuse = 3 and what hangs on it) is off, the restriction-side
 * fusions stay; fuse = 1 is bit-identical to 0 and 3 to 2. With DIRECT -- never set, or set back -- nothing changes. TE_EINVAL for
 * an unknown kind; TE_ESTATE for LINEAR on a sharded hierarchy (as above; DIRECT is untouched there). */
int te_gmg_set_interpolator(te_gmg *g, int kind);
int te_gmg_interpolator(const te_gmg *g);
/* GMG::Cycle<D>::apply(f, u) (GMG/Cycle.h:116-126) on level 0 */
int te_vcycle(te_gmg *g, const te_cycle_opts *o, const te_vec *f, te_vec *u);
/* BiCGStab<D>::solve(vg, A, x, b, Mr, max_it, tol) (BiCGStab.h:45-106). Mr = te_vcycle when
 * `o` is non-NULL. On a sharded hierarchy every rank calls it; the scalars of an iteration are summed over
 * the ranks (Vector.h:294,319) by ncclAllReduce on the solver stream (te_gmg_use_rccl) or by the
 * te_gmg_set_allreduce callback, batched as BiCGStab.h:71-97 allows: 1 + 2 + 2 doubles per iteration.
 * TE_ESTATE when several ranks exist and neither is set. */
int te_bicgstab(te_gmg *g, const te_cycle_opts *o, te_vec *x, const te_vec *b, int max_it,
                double tol, int *iterations, double *rel_resid);
/* te_bicgstab allocates its eight level-0 work vectors at its first call and keeps them for the next solve (a driver
 * solves again and again; 8 x the size of x: 8 GiB at 512^3). They are freed by te_gmg_destroy -- or by this call, for a
 * caller that has finished solving and wants the memory back (the next te_bicgstab allocates them again). */
int te_gmg_release_workspace(te_gmg *g);

/* The FMG interpolation: fine = Pi coarse. It SETS fine (it does not add), and it interpolates a SOLUTION, which carries boundary
 * data, so it reads none. The rule is TE_INTERP_LINEAR's with two changes. (1) In the extended block E, the ghost through a PHYSICAL
 * face, Dirichlet or Neumann alike, is the quadratic extrapolation 3 m - 3 m1 + m2 of the first, second and third cells inside along
 * that axis (n >= 4: they exist); faces with a neighbour keep the ghost te_apply reads (the neighbour's cell, 2 gamma - m on a
 * coarse/fine face), edges and corners the rule "sum of the face ghosts of the clamped cell, ascending axes, minus (k - 1) m".
 * (2) Per axis a, with c = (i + o_a n) >> 1 and d = -1 (i even) / +1 (i odd): v <- (30 E[c] + 5 E[c + d] - 3 E[c - d]) / 32, x then y
 * then z. With the extrapolated ghost the centred formula is the one-sided quadratic through the three innermost cells, so quadratic
 * polynomials are reproduced on every cell of a uniform hierarchy, the first and last layers included (order 3, above the operator's
 * 2, as nested iteration needs). A patch that copies through (orthant -1) receives fine = coarse bit for bit. The arguments and
 * checks of te_prolong_linear_add; makes the COARSE level's ghosts current as te_apply does; single rank (TE_ESTATE on a sharded
 * hierarchy). */
int te_prolong_quadratic(te_gmg *g, int fine_level, const te_vec *coarse, te_vec *fine);
/* Full multigrid (nested iteration): a solution of A u = f + (boundary terms) to discretisation accuracy for about the cost of a
 * few finest-level cycles, instead of te_bicgstab's solve to an algebraic tolerance. `f` is the INTERIOR right-hand side on level 0
 * with NO boundary terms folded in (the caller does not call te_add_boundary_rhs first); `bdata` the level-0 boundary vector, or
 * NULL for homogeneous data; `u` the result; cycles >= 0 the number of cycles per level (2 is enough with TE_INTERP_LINEAR and V(1,1);
 * 1, or DIRECT with 2, is not in 3D); rel_resid (may be NULL) receives |F_0 - A u|_2 / |F_0|_2.
 *   f_0 = f, b_0 = bdata; f_l+1 = te_restrict f_l, b_l+1 = te_boundary_restrict b_l; F_l = f_l + what te_add_boundary_rhs(b_l, .)
 *   adds, on EVERY level (the restriction of a folded Dirichlet term is not the coarse level's: -2 g / h^2 averages to -4 g / h_c^2);
 *   on the coarsest level, which must be ONE patch, U = the exact patch solve of F from zero (the TE_SMOOTH_PATCH_SOLVE sweep a
 *   cycle runs there under exact_coarse); then for every finer level U_l = te_prolong_quadratic U_l+1 and, `cycles` times,
 *   U_l += (one cycle with `o` and the solver's interpolator, entered at level l, on F_l - A_l U_l).
 * The work vectors (three of level 0, four of every coarser level: 3 GiB + 1/7 at 512^3) are allocated at the first call and kept;
 * te_gmg_release_workspace / te_gmg_destroy free them. The call leaves the solver's interpolator and options as they are, and a
 * te_vcycle afterwards gives the bits it gave before. On an all-Neumann hierarchy the caller supplies compatible data, as for
 * te_bicgstab, and the result is defined up to a constant. TE_EINVAL: vectors of the wrong kind, level or solver, cycles < 0;
 * TE_ESTATE: a sharded hierarchy (single rank only), or a coarsest level of more than one patch (max_levels / patches_per_proc). */
int te_fmg(te_gmg *g, const te_cycle_opts *o, const te_vec *f, const te_vec *bdata, te_vec *u, int cycles, double *rel_resid);

/* Regridding on the device: what a driver that adapts its mesh every few steps needs next to te_mesh_adapt. Neither call replaces
 * anything in the reference, which has no error indicator and never carries a solution from one mesh to another.
 *
 * te_patch_indicator: out_host[p], p = this rank's patches of `level` in local order (P_local doubles, host memory), = the largest
 * undivided second difference of u inside patch p: the maximum over the axes a, and over the cells c of the patch whose index along a
 * lies in 1 .. n-2, of |(u[c - e_a] + u[c + e_a]) - 2 u[c]|. Patch-local: no ghosts, no exchange, so it runs on sharded hierarchies
 * too (local patches). In that association the value does not depend on FMA contraction (2 u is exact) and a maximum does not depend
 * on order: the result is reproducible bit for bit. One workgroup per patch (3D levels with few patches: per z-slab, then a
 * fixed-order maximum); wave shuffles, LDS, one value per patch, no atomics. Synchronises the solver's stream. u is not modified.
 * TE_EINVAL: not a domain vector of `level` of this solver, NULL. */
int te_patch_indicator(te_gmg *g, int level, const te_vec *u, double *out_host);
/* te_vec_regrid: u_dst = the transfer of u_src from src's mesh to dst's mesh. Both are level-0 domain vectors of their solvers; the
 * solvers have the same dim and n, live on the same device and are single rank. Runs on dst's stream after a synchronisation of src's
 * stream; u_src is not modified; neither solver's state changes (a te_vcycle afterwards gives the bits it gave before). The meshes
 * must be one te_mesh_adapt apart (or the same): per destination leaf L (te_hier_leaf_tree), matched by node id and checked by
 * position and size,
 *   copy     L is a source leaf: the source patch, bit for bit.
 *   refine   L's tree parent is a source leaf X, L its orthant o, e = X's values. The extended block E on indices -1 .. n per axis is
 *            filled axis by axis, x then y then z: E[-1] = 3 e[0] - 3 e[1] + e[2], E[n] = 3 e[n-1] - 3 e[n-2] + e[n-3], later axes
 *            extrapolating the ghosts of earlier axes as well (a tensor product; EVERY patch face is treated one-sided, neighbour or
 *            not, so no ghost of the source hierarchy is read). Then, per axis a with c = (i + o_a n) >> 1 and d = -1 (i even) / +1 (i
 *            odd): v <- (30 E[c] + 5 E[c + d] - 3 E[c - d]) / 32, x then y then z -- te_prolong_quadratic's weights and march.
 *            Tensor-product quadratics are reproduced on every cell (order 3).
 *   coarsen  the 2^dim source leaves whose tree parent is L: exactly the bits te_restrict (AvgRstr.h:78-113) writes for that parent
 *            from those children.
 * The map (one row per destination patch) is built on the host at every call and uploaded. One writer per destination cell, no
 * atomics. TE_ESTATE (the message says "sharded") when either hierarchy is sharded; TE_EINVAL for NULL, a vector of the wrong kind,
 * level or solver, different n / dim / device, or a destination leaf that has no source under the three cases above -- the message
 * names its node id. */
int te_vec_regrid(te_gmg *src, const te_vec *u_src, te_gmg *dst, te_vec *u_dst);
/* te_faces_regrid: U_dst = the transfer of the FACE vector U_src (te_vec_create_faces) from src's mesh to dst's mesh, so that a
 * projected MAC velocity travels with the pressure: what te_divergence gives on dst is what it gave on src, cell by cell on copied
 * patches, on every fine cell of a refined patch the value of its coarse cell, on a coarsened patch the mean over the 2^dim fine
 * cells. Conditions as for te_vec_regrid: level-0 face vectors of their solvers, the same dim, n and device, single rank, meshes one
 * te_mesh_adapt apart (or the same); runs on dst's stream after a synchronisation of src's stream; U_src is not modified; neither
 * solver's state changes (a te_vcycle afterwards gives the bits it gave before). The map of destination leaves is te_vec_regrid's.
 * Notation: patch X has n cells per axis and spacings h_a; F_a(i; t) is component a on face plane i = 0 .. n along a at the tangential
 * cell indices t: LO_a[cell with index i along a] for i < n, HI_a[t] for i = n. Every LO_a and HI_a block of every destination patch is
 * written, by exactly one writer per entry, without atomics.
 *   copy     L is a source leaf: the source patch's dim n^dim + dim n^(dim-1) doubles, bit for bit.
 *   coarsen  L is the tree parent of 2^dim source leaves. Coarse face (a, I, t) is the mean of the 2^(dim-1) fine faces that cover it,
 *            in the child with orthant bits o_a = (I >= n/2), o_b = (t_b >= n/2) -- the mid-plane I = n/2 is the upper child's plane 0
 *            -- at fine plane 2I - o_a n and fine tangential indices 2 t_b - o_b n + {0, 1}. 3D: ((p00 + p10) + (p01 + p11)) * 0.25 with
 *            the first index along the lower remaining axis; 2D: (p0 + p1) * 0.5 (te_boundary_restrict's associations).
 *   refine   L's tree parent is a source leaf X, L its orthant o. Second order; EVERY patch edge is treated one-sidedly, neighbour or
 *            not, so no ghost of the source hierarchy is read. For b != a the tangential slope is
 *              s_ab(i; t) = (F_a(i; t + e_b) - F_a(i; t - e_b)) * 0.125,
 *            F_a extended along b by F(-1) = 3 F(0) - 3 F(1) + F(2) and F(n) = 3 F(n-1) - 3 F(n-2) + F(n-3). Fine plane i_f = 0 .. n and
 *            fine tangential indices t_f of L map to X's doubled lattice: I = i_f + o_a n, T_b = t_b + o_b n, c_b = T_b >> 1,
 *            sigma_b = -1 for T_b even and +1 for T_b odd. With
 *              G_a(i; T) = F_a(i; c) + sum_{b != a, ascending} sigma_b s_ab(i; c)
 *            the fine value is G_a(I / 2; T) for I even and, for I odd (the face lies inside coarse cell c, c_a = (I - 1) / 2),
 *              0.5 (G_a(c_a; T) + G_a(c_a + 1; T)) + sum_{b != a, ascending} 0.5 (h_a / h_b) (s_ba(c_b + 1; c) - s_ba(c_b; c)):
 *            the last term is the difference, between the coarse cell's upper and lower b-face, of component b's slope along a -- one
 *            value per coarse cell and axis, shared by the cell's 2^(dim-1) interior a-faces; h_a / h_b from X's lengths.
 *            Consequences: every fine cell's te_divergence equals its coarse cell's (to rounding); a field whose components are linear
 *            in x, y, z is reproduced; a smooth field is transferred with second-order error; the two stored copies of a face shared
 *            by two refined patches get the same bits when the source's copies agree (a face's value depends on data of its own
 *            plane only, through the same expressions; FMA contraction is off in these kernels). Where a refined patch meets a coarser
 *            one the two copies differ by construction, as for te_gradient.
 * TE_ESTATE (the message says "sharded") when either hierarchy is sharded; TE_EINVAL for NULL, a vector that is not a face vector
 * (domain, interface and boundary vectors are refused), a vector of another level or solver, the same vector as source and
 * destination, different n / dim / device, or a destination leaf without a source -- the message names its node id. */
int te_faces_regrid(te_gmg *src, const te_vec *U_src, te_gmg *dst, te_vec *U_dst);

/* The TE_* switches (docs/SWITCHES.md) are read from the environment once, in te_gmg_create. This call sets (value) or
 * clears (NULL) one of them for this solver afterwards -- how the tests pin one implementation against another. TE_ESTATE
 * for the few that shape the level tables and are therefore fixed at creation; TE_EINVAL for an unknown name. */
int te_gmg_set_option(te_gmg *g, const char *name, const char *value);

/* The number of z-slabs per patch that the 3D kernels of `level` run with right now -- the switches as they stand, TE_ZS_PIN
 * included. kind: TE_SLABS_STENCIL for the operator, residual and Jacobi kernels, the MAC operators, the interpolators, the
 * indicator and the regrid transfers; TE_SLABS_SWEEP for the RB-GS sweeps over the whole level (a launch over a part of the level,
 * as under an overlapped exchange, is ruled by the number of patches of that part). A 2D level has no slabs: 1. TE_EINVAL for
 * NULL, a level that does not exist or another kind.
 * TE_ZS_PIN = 1, 2, 4 or 8 (anything else: TE_EINVAL from te_gmg_set_option and from te_gmg_create) replaces both rules by that
 * count, clamped down to the largest one the patch size admits (n / count >= 4), whatever the number of patches. */
enum { TE_SLABS_STENCIL = 0, TE_SLABS_SWEEP = 1 };
int te_gmg_slab_count(const te_gmg *g, int level, int kind, int *zs);

/* ------------------------------------------------------------ multi-rank ghost exchange */
/* The library never talks to the network itself. When a level has off-rank neighbours, it
 * packs the needed face layers into one send buffer, calls `exchange`, and reads the receive
 * buffer. `exchange` must move, for every peer r: send[send_off[r] .. +send_cnt[r]) to rank r
 * and fill recv[recv_off[r] .. +recv_cnt[r]) from rank r (counts in doubles, device
 * pointers), ordered on `stream` (hipStream_t). This replaces the PETSc VecScatter of
 * SchurHelper.h:123-150 and GMG/InterLevelComm.h:169-189; the Python host binds it to
 * torch.distributed (RCCL) batch_isend_irecv. */
typedef int (*te_exchange_fn)(void *user, int tag, const double *send, double *recv, int npeers,
                              const int32_t *peers, const int64_t *send_off,
                              const int64_t *send_cnt, const int64_t *recv_off,
                              const int64_t *recv_cnt, void *stream);
int te_gmg_set_exchange(te_gmg *g, te_exchange_fn fn, void *user);
/* Alternative to the callback: let the library issue the exchanges itself as RCCL point-to-point
 * groups (ncclGroupStart; ncclRecv/ncclSend per peer; ncclGroupEnd) on its solver stream — the
 * direct replacement of the MPI path under the PETSc VecScatter (SchurHelper.h:123-150). `libpath`
 * names the librccl.so to dlopen (the one the host process already uses); `id128` is the 128-byte
 * ncclUniqueId produced by te_rccl_unique_id on rank 0 and broadcast by the host. */
int te_rccl_unique_id(const char *libpath, char *id128);
int te_gmg_use_rccl(te_gmg *g, const char *libpath, const char *id128, int rank, int nranks);
/* Sum (op 0) or maximum (op 1) of vals[0..n) over all ranks, in place, the same result on every rank: the
 * MPI_Allreduce of Vector.h:294,306,319 for hosts that registered an exchange callback (with te_gmg_use_rccl the
 * library reduces on the device itself). Used by te_bicgstab and te_gmg_verify_schedule. */
typedef int (*te_allreduce_fn)(void *user, double *vals, int n, int op);
int te_gmg_set_allreduce(te_gmg *g, te_allreduce_fn fn, void *user);
/* Dry run of one te_vcycle with options `o` that records every exchange each rank would issue (tag, level, peer,
 * counts) and compares, through one reduction over the ranks, what every rank sends with what its peer expects,
 * pair by pair and in order. TE_ESTATE on ALL ranks when the ranks would issue different sequences (different
 * options or hierarchies) -- instead of a hang inside RCCL in the middle of a cycle. te_vcycle runs it by itself the
 * first time it sees a set of options on a sharded hierarchy (TE_NO_VERIFY skips that). Collective.
 * With a coefficient set the dry run is the coefficient cycle's (the driver that will really run), and what has been verified is
 * remembered per options, per "a coefficient is set" and per coarse-solver kind (te_gmg_set_coef_coarse).
 * Independently, a watchdog thread ends the process (exit status 86, message on stderr) when an exchange has not
 * completed TE_EXCHANGE_TIMEOUT seconds (default 300; 0 = off) after it was issued. */
int te_gmg_verify_schedule(te_gmg *g, const te_cycle_opts *o);
/* Chooses, on the live communicator, how the sweeps of the sharded levels meet their face exchanges: everything in line on
 * the solver stream; the exchange on a second stream under the interior patches, boundary patches behind it (north star:
 * "ghost-cell exchange ... overlapped with interior smoothing"); or the interior patches on the second stream beside
 * exchange + boundary patches. Each candidate runs `reps` te_vcycle(o) behind two warm-up cycles on a scratch right-hand
 * side; the maximum over the ranks decides (one scalar reduction per candidate, so all ranks choose alike), the in-line
 * form winning ties within 2 %. All candidates give bit-identical results -- the choice changes no number. Collective;
 * call it once after te_gmg_use_rccl / te_gmg_set_exchange. *best_ms (may be NULL) = the chosen form's milliseconds per
 * cycle; report (may be NULL) receives one line with every candidate's time and the choice. Without a call the size rule
 * TE_OVERLAP_MIN decides. Replaces nothing in the reference (PETSc's VecScatterBegin/End pair, SchurHelper.h:123-150, is
 * the same idea: start the scatter, compute, finish it). */
int te_gmg_autotune(te_gmg *g, const te_cycle_opts *o, int reps, double *best_ms, char *report, int report_len);
/* A second transport for the exchanges that have a direct form (the face exchanges of 3D levels, the in-place exchange of
 * restricted blocks into a level that lives on every rank): each rank STORES what a peer needs straight into that peer's
 * receive buffer -- device memory of another process / GPU of the node, mapped through hipIpcGetMemHandle /
 * hipIpcOpenMemHandle -- and raises a flag there; a one-workgroup kernel on the receiver's stream waits for the flags. Two
 * small launches per exchange instead of an RCCL group. enable != 0: prepares it (collective; once; needs te_gmg_use_rccl or
 * te_gmg_set_allreduce, through which the handles and receive offsets are published) and switches it on; 0: switches back.
 * Results are bit-identical either way. A wait is bounded (TE_PUSH_TIMEOUT seconds; default: TE_EXCHANGE_TIMEOUT; at most 5 s inside
 * te_gmg_autotune's trial), and the kernels check the protocol themselves (csrc/pushkernels.hpp): te_gmg_push_failed returns 0, or
 * the first failure's code -- 1 a wait gave up, 2 a peer's flag was two exchanges ahead, 3 a peer was behind when its buffer was
 * overwritten, 4 this rank's epochs were out of sequence -- and the watchdog ends the process as for any exchange that never
 * completes (unless TE_PUSH_NONFATAL leaves that to the caller). A set-up that fails on one rank fails on all (the failure travels
 * with the directory reductions) and leaves nothing allocated or mapped. te_gmg_autotune, when this
 * transport has been prepared, first checks it against the other one ON THE MACHINE AT HAND (bit-identical result after a
 * cycle on different data, no wait given up, all ranks agreeing) and keeps it only if it passes and is faster.
 * The RCCL point-to-point path stays the default. Same replacement as te_gmg_use_rccl: SchurHelper.h:123-150,
 * GMG/InterLevelComm.h:169-189. */
int te_gmg_use_push(te_gmg *g, int enable);
int te_gmg_push_failed(te_gmg *g);

/* BiCGStabSolver(op, tol = 1e-12, max_it = 1000), PatchSolvers/BiCGStabSolver.h:103-108: the stopping rule of
 * TE_SMOOTH_PATCH_BCGS's patch solves (||resid|| / ||resid_0|| <= tol or max_it iterations, BiCGStab.h:69). */
int te_gmg_set_patch_bcgs(te_gmg *g, double tol, int max_it);
/* iterations each of this rank's patches of `level` took in the last TE_SMOOTH_PATCH_BCGS sweep there (its[P local], host memory;
 * synchronises the solver's stream). TE_ESTATE when no such sweep has run on the level. */
int te_gmg_patch_bcgs_iterations(te_gmg *g, int level, int32_t *its);
/* ncclCommCount / ncclCommUserRank of the communicator te_gmg_use_rccl created (0 / -1 without one): evidence for a
 * benchmark line that RCCL itself saw N ranks. */
int te_gmg_comm_info(te_gmg *g, int *rccl_nranks, int *rccl_rank);
/* moves n doubles through the active exchange back-end with this rank as its own peer (diagnostic) */
int te_gmg_exchange_selftest(te_gmg *g, int n);
/* diagnostic for the watchdog: `seconds` of exchanges enqueued without a host synchronisation (the host runs ahead of the
 * GPU; each exchange completes in milliseconds). Returns the number issued (> 0), or a TE_E* code; a watchdog that aged
 * its deadline from the first exchange instead of the oldest OUTSTANDING one would end the process with status 86 here
 * once `seconds` exceeds TE_EXCHANGE_TIMEOUT. With one rank the watchdog runs only when TE_EXCHANGE_TIMEOUT is set. */
int te_gmg_watchdog_selftest(te_gmg *g, double seconds);

/* ------------------------------------------------ Schur-complement interface route (single rank) */
/* The reference's second way to the same discrete system (apps/3d/steady.cpp:336-420, apps/2d/steady.cpp:383-480 with
 * --schur): a Krylov method on the interface values gamma alone. With Solve(f, gamma) the exact patch solves of StarPatchOp
 * with right-hand side f - 2 gamma / h^2 on the face layers and Interp the interpolation to the interfaces:
 *   T gamma = Interp(Solve(0, gamma)),  S = I - T,  g = Interp(Solve(f, 0));  S gamma* = g,  u = Solve(f, gamma*) solves A u = f.
 * gamma / x / y are interface vectors (te_vec_create_iface), u / f domain vectors, all of `level`. Every call returns TE_ESTATE
 * on a sharded hierarchy. DESIGN.md "Schur-complement route" has the kernels. */
/* SchurHelper<D>::interpolateToInterface (SchurHelper.h:333-343): gamma = Interp(u) */
int te_iface_interp(te_gmg *g, int level, const te_vec *u, te_vec *gamma);
/* SchurHelper<D>::applyWithInterface (SchurHelper.h:344-359, StarPatchOp.h:28-184): f = A_patch u with the interface
 * values gamma on every face that has a neighbour */
int te_apply_with_interface(te_gmg *g, int level, const te_vec *u, const te_vec *gamma, te_vec *f);
/* PatchOperator<D>::addInterfaceToRHS (StarPatchOp.h:185-203), in place: f -= 2 gamma / h^2 on the face layers */
int te_add_iface_rhs(te_gmg *g, int level, const te_vec *gamma, te_vec *f);
/* SchurHelper<D>::solveWithInterface (SchurHelper.h:280-297): u = Solve(f, gamma); diff (may be NULL) = Interp(u) - gamma */
int te_solve_with_interface(te_gmg *g, int level, const te_vec *f, te_vec *u, const te_vec *gamma, te_vec *diff);
/* Operators/SchurWrapOp.h with the identity term the Schur system needs: y = x - T x (x and y distinct) */
int te_schur_apply(te_gmg *g, int level, const te_vec *x, te_vec *y);
/* PolyChebPrec::apply (PolyChebPrec.cpp): y = p(T) x, p the degree-15 Chebyshev approximation of 1 / (1 - t) on
 * [0, 0.95] (coefficients from their closed form), by the same Clenshaw recurrence: an approximation of S^-1 */
int te_schur_cheb(te_gmg *g, int level, const te_vec *x, te_vec *y);
#define TE_SCHUR_PREC_NONE 0
#define TE_SCHUR_PREC_CHEB 1
/* BiCGStab<D-1>::solve (BiCGStab.h:45-106, the statements of te_bicgstab) on S gamma = g, right-preconditioned by `prec`;
 * gamma = the initial guess on entry, the solution on exit; then u = Solve(f, gamma). Stops when ||r|| / ||r0|| <= tol
 * or after max_it iterations. A level without interfaces (one patch) takes 0 iterations: u = Solve(f, -). */
int te_schur_solve(te_gmg *g, int level, int prec, const te_vec *f, te_vec *u, te_vec *gamma, int max_it, double tol,
                   int *iterations, double *rel_resid);

/* Domain<D>::integrate (Domain.h:258-278) and Domain<D>::volume (:237-251), this rank's part (the host adds the
 * ranks as it does for norms): sum over local patches of (sum of the patch's cells) * (cell volume), resp. of the
 * patch volumes. What the drivers need for pure-Neumann problems (apps/3d/steady.cpp:330-334, 539-549).
 * A level that lives on EVERY rank (te_hier_level_replicated) is counted once: rank 0 returns the whole level, every other
 * rank 0.0, so that the sum over the ranks is the level's integral / volume as on any other level. The same holds for
 * te_vec_two_norm_sq and te_vec_dot on such a level (te_vec_inf_norm returns the level's value on every rank: a maximum
 * over the ranks is unchanged). */
int te_integrate(te_gmg *g, int level, const te_vec *v, double *out);
int te_volume(te_gmg *g, int level, double *out);

/* Init::initDirichlet / Init::initNeumann (apps/shared/Init.cpp:152-245, :57-151; 2D :246-361) for the drivers'
 * canned problems, evaluated on the device straight into `f` and (may be NULL) `exact`: right-hand side and exact
 * solution at the cell centres, physical Dirichlet data folded in as -2 g/h^2, Neumann data as +-g_n/h, in the
 * reference's face order. TE_PROBLEM_TRIG / TE_PROBLEM_GAUSS are apps/3d/steady.cpp:221-292 (2D: apps/2d/steady.cpp:296-318);
 * TE_PROBLEM_RANDOM is the timing input f ~ U(-1,1) from splitmix64(0x5EED + tree node id) (exact := 0). Arbitrary
 * std::function problems go through Vector<D>::getLocalData (thunderegg/HipInit.h). */
#define TE_PROBLEM_TRIG 0
#define TE_PROBLEM_GAUSS 1
#define TE_PROBLEM_RANDOM 2
int te_init_problem(te_gmg *g, int level, int problem, int neumann, te_vec *f, te_vec *exact);

/* The boundary half of Init::initDirichlet / Init::initNeumann (apps/shared/Init.cpp:186-240, :89-146) with the data taken from a
 * boundary vector, in place, on the device: on a Dirichlet face f -= 2 g / h^2, on a Neumann face f += g_n / h (lower side) or
 * f -= g_n / h (upper side), g_n the derivative ALONG THE AXIS (Init.cpp's nfunx / nfuny / nfunz, not the outward normal), h the
 * patch's spacing on that axis. Cells on edges and corners receive one term per physical side, in side order. Touches the face
 * layers of boundary patches only; deterministic (no atomics). */
int te_add_boundary_rhs(te_gmg *g, int level, const te_vec *bdata, te_vec *f);
/* the canned problems' boundary data (TE_PROBLEM_TRIG / TE_PROBLEM_GAUSS): the exact solution at the face points of Dirichlet faces,
 * its derivative along the axis on Neumann faces -- what te_init_problem_sides folds in */
int te_boundary_sample(te_gmg *g, int level, int problem, te_vec *bdata);
/* The boundary vector of the next coarser level: each entry of a coarse physical-face block is the mean of the 2^(dim-1) fine face
 * entries that cover it -- 3D ((a + b) + (c + d)) * 0.25 with a, b adjacent along the face's lower remaining axis, 2D (a + b) * 0.5 --
 * from the block of the child whose orthant bits on the face's remaining axes name that quadrant; a patch that copies through hands
 * its blocks on bit for bit. Dirichlet values and Neumann derivatives restrict alike. fine_bdata: a boundary vector of fine_level,
 * coarse_bdata: one of fine_level + 1 (TE_EINVAL otherwise). One writer per entry, deterministic. Single rank (TE_ESTATE on a
 * sharded hierarchy). Folding the result with te_add_boundary_rhs gives the coarse level's boundary terms; restricting a FOLDED
 * right-hand side does not (twice the Dirichlet term). */
int te_boundary_restrict(te_gmg *g, int fine_level, const te_vec *fine_bdata, te_vec *coarse_bdata);
/* te_init_problem with the kind of every physical face taken from the hierarchy's side mask (te_hier_build_bc) instead of one flag:
 * Init::initDirichlet's term on Dirichlet faces and Init::initNeumann's on Neumann faces in one pass (for mask 0 / all bits the
 * very bits of te_init_problem with neumann = 0 / 1). */
int te_init_problem_sides(te_gmg *g, int level, int problem, te_vec *f, te_vec *exact);

/* The operators that turn a pressure into a velocity correction, consistent with te_apply's discrete Laplacian (a flow solver's
 * projection step: f = div(u*) / dt before the solve, u = u* - dt grad(p) after it). They replace nothing in the reference.
 * h_a = the patch's spacing on axis a, m = the cell just inside a patch face:
 *   G = grad u     interior face between cells c - e_a and c: (u[c] - u[c - e_a]) / h_a; patch face with a neighbour: (m - ghost) / h_a
 *                  below, (ghost - m) / h_a above, ghost = exactly the value te_apply uses there (same level: the neighbour's cell,
 *                  local or received; coarse/fine: 2 gamma - m with TriLinInterp / BilinearInterpolator's gamma); physical Dirichlet
 *                  face: ghost = 2 g - m; physical Neumann face: G = g_n. g / g_n come from the boundary vector `bdata` of the same
 *                  level (NULL: zero).
 *   out = alpha div U    out[c] = alpha * sum_a (U_a(upper a-face of c) - LO_a[c]) / h_a; patch-local, no exchange.
 *   U -= alpha grad p    te_project: one fused pass, the gradient is never stored.
 * te_divergence(1, te_gradient(u, bdata)) equals te_apply(u) minus what te_add_boundary_rhs(bdata, .) adds to a zero vector, up to
 * rounding. Both copies of a same-level face receive the same bits (one rank or several); on a coarse/fine face the two sides differ
 * by construction (the operator is not flux-matched there). te_gradient and te_project are collective on a sharded hierarchy (they
 * make the ghosts current as te_apply does); te_divergence is local. TE_EINVAL: NULL, another solver's or level's vector, a vector
 * of the wrong kind (u, p, out: domain vectors; G, U: face vectors; bdata: a boundary vector or NULL). */
int te_gradient(te_gmg *g, int level, const te_vec *u, const te_vec *bdata, te_vec *G);
int te_divergence(te_gmg *g, int level, double alpha, const te_vec *U, te_vec *out);
int te_project(te_gmg *g, int level, double alpha, const te_vec *p, const te_vec *bdata, te_vec *U);

/* The variable-coefficient operator A_b u = div(beta grad u): the pressure equation of a flow with variable density,
 * div((1 / rho) grad p) = div(u*) / dt. Nothing in the reference has it. A second, unfused path next to the Laplacian's, taken only
 * while a coefficient is set; with none set every call gives the bits it gave before these entry points existed.
 *
 * SHARDED HIERARCHIES. te_faces_restrict, te_gmg_set_coefficient, te_gmg_set_reaction, te_gmg_set_coef_coarse,
 * te_vcycle with a coefficient (TE_INTERP_DIRECT only), te_bicgstab with a coefficient and te_project_weighted are COLLECTIVE: every
 * rank calls them, in the same order, each with the entries of its own patches. te_apply, te_residual, te_residual_norm_sq (this
 * rank's part, as on the Laplacian path) and te_smooth with a coefficient are collective as they are without one. Results equal the
 * single-rank run bit for bit: a child whose parent lives on another rank restricts its own block of beta and ships it, through the
 * attached back-end (te_gmg_use_rccl or te_gmg_set_exchange; never the direct-store transport, which keeps serving the face
 * ghosts). The collective set calls return TE_ESTATE (the message says "sharded") while NO transport is attached. Still single rank:
 * TE_INTERP_LINEAR, te_fmg, te_patch_apply with a coefficient, the Schur route, te_faces_from_cells.
 *
 * beta is a FACE vector of the level (te_vec_create_faces: per patch LO_a then HI_a). A face shared by two patches is stored by
 * both: the caller keeps the two copies equal and every entry > 0; nothing checks this. rh2_a = 1 / h_a^2. u_lo / u_hi = the cell's
 * neighbours along axis a; across a patch face exactly the ghost te_apply reads there: the neighbour's cell, 2 gamma - m on a
 * coarse/fine face, -m on a physical Dirichlet face, +m on a Neumann face (m = the cell just inside). b_lo / b_hi = beta on the cell's
 * lower / upper a-face: LO_a[c], and LO_a[c + e_a] or HI_a on the patch's upper face.
 *   operator   (A_b u)[c] = sum over a = x, y, z in that order of (b_hi (u_hi - u_c) - b_lo (u_c - u_lo)) * rh2_a; up to rounding
 *              te_divergence(1, beta (.) te_gradient(u, NULL)).
 *   residual   r = f - A_b u.
 *   RB-GS      patch-local, red = (x + y + z) even first; ghosts of faces with a neighbour frozen at the old iterate, coarse/fine
 *              included. u_c <- (o - f_c) / d; o = sum over sides of b_s v_s rh2_a over interior neighbours and frozen ghosts
 *              (physical faces contribute 0); d = sum over sides of b_s kappa_s rh2_a, kappa = 1 (interior or neighbour face),
 *              2 (physical Dirichlet), 0 (physical Neumann). With beta = 1 the constant-coefficient sweep's numbers.
 *   Jacobi     u <- u + omega (f - A_b u) / (-d_J), d_J = sum over sides of b_s (1 + adj_s) rh2_a; adj_s on a patch face: physical
 *              Dirichlet +1, Neumann -1, this patch the fine side of a coarse/fine face -5/6 (3D) / -2/3 (2D), the coarse side +1/3;
 *              anything else 0.
 *   coarse levels   level l + 1's beta = the face average of level l's (te_faces_regrid's "coarsen" rule between the levels of one
 *              hierarchy): coarse face (a, I, t) = the mean of the 2^(dim-1) fine faces that cover it, in the child with orthant bits
 *              o_a = (I >= n/2), o_b = (t_b >= n/2) at fine plane 2 I - o_a n (the mid-plane is the upper child's plane 0);
 *              3D ((p00 + p10) + (p01 + p11)) * 0.25, 2D (p0 + p1) * 0.5 (te_boundary_restrict's associations). A patch that copies
 *              through hands its blocks on bit for bit. One writer per entry, no atomics.
 *
 * te_faces_restrict: coarse = that average of fine; face vectors of fine_level and fine_level + 1 (TE_EINVAL otherwise). Collective
 * on a sharded hierarchy; TE_ESTATE (the message says "sharded") there while no transport is attached.
 * te_gmg_set_coefficient: beta = a level-0 face vector of this solver (TE_EINVAL otherwise). The solver COPIES it (the caller may free
 * or overwrite its vector) and restricts it level by level. The per-level copies are allocated at the first call and reused (a driver
 * calls this every time step); te_gmg_destroy frees them. NULL clears the coefficient and keeps the buffers;
 * te_gmg_release_workspace frees them too, but only while cleared. Collective on a sharded hierarchy (beta = this rank's patches;
 * the send and receive buffers of the blocks that travel are made at the first such call and freed with the copies); TE_ESTATE
 * ("sharded") there while no transport is attached (NULL is always accepted). A call that fails after its checks leaves NO
 * coefficient set, never a partly updated one.
 * te_gmg_has_coefficient: 0 or 1. te_gmg_coefficient: out = the level's beta (a face vector of that level: this rank's patches, on a
 * level that lives on every rank all of it); TE_ESTATE when none is set.
 *
 * While a coefficient is set:
 *   te_apply, te_residual, te_residual_norm_sq use A_b (the norm is a second pass over r).
 *   te_smooth takes TE_SMOOTH_RBGS and TE_SMOOTH_JACOBI; TE_SMOOTH_PATCH_SOLVE and TE_SMOOTH_PATCH_BCGS return TE_EUNSUPPORTED (their
 *   patch solves invert the constant-coefficient patch operator).
 *   te_vcycle runs a plain driver, GMG/Cycle.h:56-126 statement for statement: V and W, pre / mid / post / coarse sweeps, the solver's
 *   interpolator (DIRECT or LINEAR), te_restrict's restriction. `fuse` is IGNORED (every value gives the same bits). `exact_coarse`
 *   is IGNORED: the coarsest level runs coarse_sweeps sweeps of o->smoother -- a coarsest level of ONE patch wants coarse_sweeps of
 *   the order of a few n (n = cells per axis) to be solved well enough. Other smoothers: TE_EUNSUPPORTED.
 *   te_bicgstab applies A_b and preconditions with that cycle (its separate-pass form, what TE_NO_BICG_FUSE selects).
 *   te_fmg, te_patch_apply and every call of the Schur route (te_iface_interp ... te_schur_solve) return TE_ESTATE; the message
 *   contains "coefficient".
 *   te_gradient, te_divergence, te_project, te_restrict, the prolongations, the BLAS-1 calls, the boundary and the regrid calls never
 *   involve beta and are unchanged. te_add_boundary_rhs folds the CONSTANT-coefficient terms: with a coefficient the right-hand-side
 *   terms of boundary data are -te_divergence(1, beta (.) te_gradient(0, bdata)), or in one call
 *   te_add_boundary_rhs_weighted(bdata, beta, .) below.
 *
 * Every call of te_gmg_set_coefficient, with beta or with NULL, CLEARS the reaction term sigma (te_gmg_set_reaction below): the order
 * per time step is beta, then sigma. */
int te_faces_restrict(te_gmg *g, int fine_level, const te_vec *fine, te_vec *coarse);
int te_gmg_set_coefficient(te_gmg *g, const te_vec *beta);
int te_gmg_has_coefficient(const te_gmg *g);
int te_gmg_coefficient(te_gmg *g, int level, te_vec *out);

/* The reaction term: A_bs u = div(beta grad u) - sigma u, the operator of an implicit viscous or diffusive step
 * (rho / dt) u - div(mu grad u) = rhs, in this library's sign convention div(mu grad u) - (rho / dt) u = -rhs: beta = mu,
 * sigma = rho / dt, f = -rhs. sigma lives on the variable-coefficient path only. Collective on a sharded
 * hierarchy (te_restrict's blocks travel as they do for a residual).
 *
 * sigma is a CELL vector of the level (te_vec_create's layout), every entry >= 0; nothing checks this, exactly as with beta.
 *   operator   (A_bs u)[c] = (A_b u)[c] - sigma_c u_c: A_b evaluated exactly as written above, then one multiplication and one
 *              subtraction. Residual r = f - A_bs u.
 *   RB-GS      u_c <- (o - f_c) / (d + sigma_c), o and d as above; colour order and frozen ghosts unchanged.
 *   Jacobi     u <- u + omega (f - A_bs u) / (-(d_J + sigma_c)).
 *   coarse levels   level l + 1's sigma = te_restrict's average of level l's; a patch that copies through hands its block on bit
 *              for bit.
 *
 * te_gmg_set_reaction: sigma = a level-0 cell vector of this solver (TE_EINVAL for a face, interface or boundary vector, another
 * level's or another solver's). The solver COPIES it and restricts it to every level, into per-level cell vectors allocated at the
 * first call and reused (a driver calls this every time step). NULL clears sigma and keeps the buffers. TE_ESTATE (the message says
 * "coefficient") unless a coefficient is set; TE_ESTATE ("sharded") on a sharded hierarchy without a transport. A call that fails after its checks
 * leaves NO sigma set. ORDER: every te_gmg_set_coefficient clears sigma, so per time step call te_gmg_set_coefficient first, then
 * te_gmg_set_reaction -- the operator is always what the last calls said, never a new beta with a stale sigma.
 * te_gmg_release_workspace frees the sigma buffers while sigma is cleared (and everything of the coefficient while that is
 * cleared); te_gmg_destroy always.
 * te_gmg_has_reaction: 0 or 1. te_gmg_reaction: out = the level's sigma (a cell vector of that level: this rank's patches); TE_ESTATE
 * when none is set.
 *
 * While sigma is set te_apply, te_residual, te_residual_norm_sq, te_smooth (RB-GS, Jacobi), te_vcycle (V and W, both interpolators)
 * and te_bicgstab use A_bs; everything refused with a coefficient stays refused with the same codes. With sigma > 0 somewhere the
 * all-Neumann problem is nonsingular.
 *
 * Constant viscosity, Laplace(u) - sigma u = f: create a face vector, te_vec_set(beta, 1.0), te_gmg_set_coefficient(g, beta), then
 * te_gmg_set_reaction(g, sigma).
 * Boundary data: sigma multiplies no ghost, so the right-hand-side terms of inhomogeneous data are those of A_b, unchanged:
 * -te_divergence(1, beta (.) te_gradient(0, bdata)). */
int te_gmg_set_reaction(te_gmg *g, const te_vec *sigma);
int te_gmg_has_reaction(const te_gmg *g);
int te_gmg_reaction(te_gmg *g, int level, te_vec *out);

/* The coarsest level of the variable-coefficient cycle. By default te_vcycle with a coefficient runs
 * coarse_sweeps sweeps there (TE_COEF_COARSE_SWEEPS). With TE_COEF_COARSE_SUBCYCLE a coarsest level of ONE patch of n^D cells is solved
 * by multigrid again: it is the same grid as a uniform tree of (n / sub_n)^D patches of sub_n^D cells, on which the path's own kernels
 * and its own coarse levels exist. In place of the coarse_sweeps loop:
 *   1. f and the incoming u of the one-patch level are split into the level-0 vectors of an AUXILIARY solver on a root of the same
 *      lengths and per-side boundary kinds, log2(n / sub_n) uniform refinements, patch size sub_n;
 *   2. that solver's cycle (the driver above, u carried, not zeroed) runs `cycles` times with the caller's te_cycle_opts -- smoother,
 *      pre / mid / post sweeps, cycle type, omega, and coarse_sweeps, which now counts sweeps on the one sub_n^D patch -- and the
 *      parent's interpolator at that moment;
 *   3. u is merged back.
 * The auxiliary level-0 beta and sigma are the split of the parent's coarsest-level beta and sigma: a patch's LO block is the matching
 * block of the big patch's LO; its HI is the big LO plane at offset + sub_n, or the big HI on the big patch's upper face (the two
 * copies of a shared face are equal by construction). Below that the auxiliary solver restricts as te_gmg_set_coefficient /
 * te_gmg_set_reaction do. Every te_gmg_set_coefficient and te_gmg_set_reaction of the parent refreshes them, and so does
 * te_gmg_set_coef_coarse itself when a coefficient is set; "beta first, then sigma; every beta clears sigma" holds for both solvers.
 *
 * The setting is a property of the SOLVER, not of a coefficient: it may be made with or without beta set and survives every
 * te_gmg_set_coefficient, NULL included. The default is TE_COEF_COARSE_SWEEPS; until the call is made nothing changes. te_smooth on
 * the coarsest level is untouched. A hierarchy of one level is allowed (te_vcycle is then the sub-solve alone). No silent fallback:
 * what te_gmg_coef_coarse reports is what runs.
 *
 * sub_n is valid if it is even, >= 4, in 3D one of 4, 8, 16, and n / sub_n is a power of two >= 2. sub_n = 0 picks one: in 3D 8 where
 * that is valid (the measured choice: DESIGN.md section 20), otherwise the smallest valid value, which is 4 where 4 is valid.
 * te_gmg_set_coef_coarse returns
 *   TE_EINVAL        unknown kind, cycles < 1, an invalid explicit sub_n;
 *   TE_ESTATE        a sharded hierarchy with no transport attached (the message says "sharded");
 *   TE_EUNSUPPORTED  the coarsest level has more than one patch (a truncated hierarchy; the message carries the count), or no valid
 *                    sub_n exists (n = 4 in 3D; in 2D an n whose halves never reach an even size >= 4, e.g. no multiple of 4);
 * and changes nothing then. With TE_COEF_COARSE_SWEEPS only kind and cycles are checked (sub_n is not used).
 * The auxiliary mesh, hierarchy and solver belong to the parent: made by the first TE_COEF_COARSE_SUBCYCLE call (again when sub_n
 * changes), on the parent's stream; te_gmg_release_workspace frees them while the kind is TE_COEF_COARSE_SWEEPS, te_gmg_destroy always.
 * te_gmg_profile and its companions act on the auxiliary solver too; its launches are counted in the parent's rows under their
 * existing names, the split and the merge as "coef_split" and "coef_merge".
 * te_gmg_coef_coarse: the current kind, the RESOLVED sub_n (0 while no sub-cycle has been selected) and cycles; NULL outputs are skipped.
 * Sharded hierarchies: every rank calls te_gmg_set_coef_coarse and gets the same code (the patch count is the GLOBAL one). The auxiliary
 * solver is single rank and exchanges nothing; a rank builds and runs it exactly when it holds the one coarsest patch -- every rank
 * where that level lives on every rank, its owner otherwise -- and a rank without the patch does nothing at that point of the cycle. */
#define TE_COEF_COARSE_SWEEPS   0 /* default: coarse_sweeps sweeps on the coarsest level */
#define TE_COEF_COARSE_SUBCYCLE 1
int te_gmg_set_coef_coarse(te_gmg *g, int kind, int sub_n, int cycles);
int te_gmg_coef_coarse(const te_gmg *g, int *kind, int *sub_n, int *cycles);

/* A variable-density projection step on the device: rho (or mu) stays a CELL vector, the face coefficient is built from it here, the
 * boundary terms of the right-hand side are folded under it, and the velocity correction u = u* - dt beta grad p is one pass. All three
 * calls are additive: none reads or changes the coefficient of te_gmg_set_coefficient, and a te_vcycle afterwards gives the bits it
 * gave before.
 *
 * te_faces_from_cells(g, level, mode, c, cb, F): c = a domain vector of `level`, cb = a boundary vector of `level` or NULL, F = a face
 * vector of `level`. Every LO_a / HI_a entry of every patch is written by exactly one writer, no atomics. A face has two operands: lo,
 * the value on its lower-coordinate side, and hi, the value on its upper side.
 *   TE_FACE_MEAN        (lo + hi) * 0.5                 (a viscosity)
 *   TE_FACE_HARMONIC    (2.0 * (lo * hi)) / (lo + hi)
 *   TE_FACE_RECIP_MEAN  2.0 / (lo + hi)                 (beta = 1 / rho_face)
 *   interior face, patch face with a same-level neighbour: the two adjacent cells, the neighbour's read in place; both stored copies of
 *     such a face receive the same bits in every mode.
 *   physical face (Dirichlet and Neumann alike: the coefficient field has no boundary condition of its own): v = cb's entry for that face
 *     point where cb is given, else the cell just inside; the result is v bit for bit (MEAN, HARMONIC) or 1.0 / v (RECIP_MEAN).
 *   coarse/fine face: plain averages, not the operator's ghost 2 gamma - m (gamma carries weights of -1/12 and can go negative across a
 *     jump). Fine side: the other operand is the coarse neighbour's cell of its facing layer that covers the face, at
 *     ((a + (q & 1 ? n : 0)) / 2, (b + (q & 2 ? n : 0)) / 2), q = this patch's quadrant on the coarse face. Coarse side: the other operand is
 *     ((f00 + f10) + (f01 + f11)) * 0.25 over the four fine cells of the facing layer that cover the coarse cell, first index along the
 *     face's lower remaining axis (2D: (f0 + f1) * 0.5). The two copies differ by construction, as for te_gradient; in MEAN mode the coarse
 *     copy equals the mean of the four fine copies up to rounding.
 * All operands must be > 0 for the two division modes; nothing checks this, exactly as for beta. Works on every level.
 * ORDER OF ACCURACY. Without cb the coefficient on a physical face is the inner cell's value, an O(h) error there. That is harmless where
 * the flux datum on that face is zero (walls) or the face is Dirichlet (the solve stays second order), and FIRST order where an
 * inhomogeneous Neumann datum g_n != 0 meets it: pass the wall values of the field in cb then (second order again).
 * TE_EINVAL: NULL (c, F), a vector of the wrong kind, level or solver, an unknown mode. TE_ESTATE (the message says "sharded") on a
 * sharded hierarchy.
 *
 * te_project_weighted(g, level, alpha, p, bdata, w, U): U <- U - alpha (w (.) grad p) in one pass, the gradient never stored. G is
 * exactly te_gradient(p, bdata)'s value (the same ghosts; on a physical Neumann face g_n itself); t = w * G is one multiplication, then
 * U = fma(-alpha, t, U). With w = 1 everywhere the call gives te_project's bits; both copies of a same-level face get the same bits when
 * w's (and U's) copies agree. w = a face vector of the level, distinct from U. TE_EINVAL: w aliases U, wrong kinds, levels or solvers.
 * Collective on a sharded hierarchy, as te_project is (bit for bit the single-rank result); TE_ESTATE ("sharded") there while no
 * transport is attached.
 *
 * te_add_boundary_rhs_weighted(g, level, bdata, w, f): te_add_boundary_rhs with every datum multiplied first by w on its physical face,
 * b <- w_face * b (w_face = LO_a of the layer's cell on a lower side, HI_a on an upper side), then the same expressions: Dirichlet
 * f -= 2 b / (h h), Neumann f += b / h below, f -= b / h above; the same owner rule, side order and one writer per cell. With w = 1 the
 * bits of te_add_boundary_rhs; up to rounding -te_divergence(1, w (.) te_gradient(0, bdata)), the boundary terms under A_b with
 * beta = w. Patch-local: runs on a sharded hierarchy like te_add_boundary_rhs. TE_EINVAL: wrong kinds, levels or solvers. */
#define TE_FACE_MEAN       0
#define TE_FACE_HARMONIC   1
#define TE_FACE_RECIP_MEAN 2
int te_faces_from_cells(te_gmg *g, int level, int mode, const te_vec *c, const te_vec *cb, te_vec *F);
int te_project_weighted(te_gmg *g, int level, double alpha, const te_vec *p, const te_vec *bdata, const te_vec *w, te_vec *U);
int te_add_boundary_rhs_weighted(te_gmg *g, int level, const te_vec *bdata, const te_vec *w, te_vec *f);

/* Transport of a cell field by a face velocity on the device: rho^{n+1} = rho^n - dt div(U rho) with the projected velocity U, first
 * order upwind (donor cell), conservative on refined meshes. The four calls work on every level, in 2D and 3D, and are additive: none
 * reads or changes the solver's coefficient, reaction term, interpolator or options, and a te_vcycle or te_bicgstab afterwards gives the
 * bits it gave before. Single rank: TE_ESTATE (the message says "sharded") on a sharded hierarchy.
 *
 * te_advect_flux(g, level, U, c, cb, F): F = U (.) c_upwind. U, F = distinct face vectors of `level`, c = a domain vector, cb = a
 * boundary vector of `level` or NULL. Every entry has one writer, no atomics. A face has two operands, lo on its lower-coordinate side
 * and hi on its upper side, and with U = this patch's own stored entry of the face
 *     s = (U >= 0.0) ? lo : hi,   F = U * s.
 *   interior face, patch face with a same-level neighbour: the two adjacent cells, the neighbour's read in place (te_faces_from_cells'
 *     operands); both stored copies of such a face receive the same bits when U's copies agree.
 *   physical face (Dirichlet and Neumann alike): outside the domain stands cb's entry for that face point where cb is given, else the
 *     cell just inside; inside stands that cell. Inflow carries the datum, outflow the cell's own value.
 *   coarse/fine face, fine side: the other operand is the coarse neighbour's cell that covers the face (te_faces_from_cells' rule), the
 *     entry is formed as above with the fine copy of U.
 *   coarse/fine face, coarse side: ((F00 + F10) + (F01 + F11)) * 0.25 (2D: (F0 + F1) * 0.5) of the fine-side fluxes of the fine faces
 *     that cover the coarse face, first index along the face's lower remaining axis. They are formed from the fine patches' own copies
 *     of U, their facing-layer cells and this coarse cell -- the operands and the expression of the fine side -- so the coarse copy
 *     equals the mean of the fine copies BIT FOR BIT: te_divergence(F) telescopes across the face. The coarse copy of U there is never
 *     read.
 * TE_EINVAL: NULL (U, c, F), a vector of the wrong kind, level or solver, F aliases U.
 *
 * te_advect(g, level, alpha, U, c, cb, out): out = c - alpha div(U c_upwind) in one pass, the flux never stored. out = a domain vector
 * distinct from c. The bits are those of the composition te_advect_flux -> F, d = te_divergence(alpha, F), te_vec_copy(out, c),
 * te_vec_add_scaled(out, -1.0, d). With alpha * dim * rate <= 1 (rate: te_faces_max_rate of U) and c, cb >= 0 the result is >= 0.
 * TE_EINVAL: NULL (U, c, out), wrong kinds, levels or solvers, out aliases c.
 *
 * te_faces_match(g, level, F): on every coarse/fine face the coarse side's stored entries become the mean of the covering fine copies
 * (the association above); everything else is untouched. One writer per entry, no atomics. Afterwards te_divergence(F) telescopes across
 * coarse/fine faces -- for any face field, e.g. a projected velocity before it transports something. Idempotent; te_advect_flux's
 * output is a fixed point, bit for bit. TE_EINVAL: NULL, not a face vector of the level.
 *
 * te_faces_max_rate(g, level, U, rate): *rate = the maximum over all stored entries of |U_a| / h_a, h_a the owning patch's spacing
 * (0 on a level without patches). Synchronises the solver stream. TE_EINVAL: NULL, not a face vector of the level. */
int te_advect_flux(te_gmg *g, int level, const te_vec *U, const te_vec *c, const te_vec *cb, te_vec *F);
int te_advect(te_gmg *g, int level, double alpha, const te_vec *U, const te_vec *c, const te_vec *cb, te_vec *out);
int te_faces_match(te_gmg *g, int level, te_vec *F);
int te_faces_max_rate(te_gmg *g, int level, const te_vec *U, double *rate);

/* Second-order limited (MUSCL) transport: te_advect_flux / te_advect with the cell operands of a face replaced by edge states formed
 * from limited slopes. Every level, 2D and 3D, additive like the calls above; single rank: TE_ESTATE ("sharded")
 * on a sharded hierarchy. Every operation below is rounded on its own.
 *
 * Slope of a cell along axis a: dm = c - m and dp = p - c, with m and p the operands beyond the cell's lower and upper a-face. The
 * operand beyond a face is exactly te_faces_from_cells' and te_advect_flux's: the same-level neighbour's facing cell; on a physical
 * face the boundary vector's entry, or without cb the cell itself; the covering coarse cell, raw, where the neighbour is coarser; the
 * average ((f00 + f10) + (f01 + f11)) * 0.25 (2D (f0 + f1) * 0.5) of the covering fine cells where the neighbours are finer.
 *   TE_SLOPE_ZERO (0)      S = 0.0
 *   TE_SLOPE_MINMOD (1)    S = (dm*dp > 0.0) ? (fabs(dm) < fabs(dp) ? dm : dp) : 0.0
 *   TE_SLOPE_MC (2)        t = 0.5*(dm + dp), w = fmin(fmin(2.0*fabs(dm), 2.0*fabs(dp)), fabs(t)), S = (dm*dp > 0.0) ? copysign(w, dm) : 0.0
 *   TE_SLOPE_CENTRAL (3)   S = 0.5*(dm + dp). Unlimited, no positivity guarantee: for smooth fields, and the tests' negative control.
 *
 * Flux of a face: te_advect_flux's rule, s = (U >= 0.0) ? lo : hi, F = U * s, with the cell operands replaced by edge states. A cell
 * on the lower side of the face contributes lo = c + 0.5*S_a, a cell on the upper side hi = c - 0.5*S_a. An operand that is not a cell
 * of this level enters as it is: the boundary datum, the own cell standing in for it, the raw coarse cell on the fine side of a
 * coarse/fine face, and the coarse cell on the coarse side.
 *   same-level interior face: both sides are edge states; the two patches' copies get the same bits when U's copies agree.
 *   coarse/fine face, fine side: upwindFlux(U_f, C, m - 0.5*S) on a lower face, upwindFlux(U_f, m + 0.5*S, C) on an upper one; C the
 *     covering coarse cell, m the fine facing cell, S its slope along the face's axis.
 *   coarse/fine face, coarse side: the mean (te_advect_flux's association) of those same fine-side values, formed from the fine patch's
 *     own U, m, S and this C: the coarse copy equals the mean of the fine copies bit for bit. The coarse copy of U is never read.
 * The scheme is first order at coarse/fine and physical faces and second order elsewhere.
 *
 * te_cell_slopes(g, level, kind, c, cb, sx, sy, sz): the slopes of c along x, y, z. sx, sy, sz = distinct domain vectors of `level`,
 * none aliasing c; sz is NULL in 2D and required in 3D. c is read once.
 * te_advect_flux_muscl(g, level, kind, U, c, cb, F), te_advect_muscl(g, level, alpha, kind, U, c, cb, out): te_advect_flux's and
 * te_advect's arguments and refusals, plus TE_EINVAL for an unknown kind. The slopes live in vectors the solver owns per level, made at
 * first use and freed by te_gmg_release_workspace and te_gmg_destroy. te_advect_muscl's bits are those of te_advect_flux_muscl -> F,
 * d = te_divergence(alpha, F), te_vec_copy(out, c), te_vec_add_scaled(out, -1.0, d). With TE_SLOPE_ZERO both give te_advect_flux's and
 * te_advect's values. For ZERO, MINMOD and MC, with c, cb >= 0 and ANY U: alpha * 2 * dim * rate <= 1 keeps the result >= 0 on a level
 * without coarse/fine faces, alpha * 2.5 * dim * rate <= 1 on one with them (rate: te_faces_max_rate of U). */
#define TE_SLOPE_ZERO    0
#define TE_SLOPE_MINMOD  1
#define TE_SLOPE_MC      2
#define TE_SLOPE_CENTRAL 3
int te_cell_slopes(te_gmg *g, int level, int kind, const te_vec *c, const te_vec *cb, te_vec *sx, te_vec *sy, te_vec *sz);
int te_advect_flux_muscl(te_gmg *g, int level, int kind, const te_vec *U, const te_vec *c, const te_vec *cb, te_vec *F);
int te_advect_muscl(te_gmg *g, int level, double alpha, int kind, const te_vec *U, const te_vec *c, const te_vec *cb, te_vec *out);

/* kernel timing hooks for bench.py: HIP-event time of the last te_vcycle's dominant kernel */
int te_gmg_profile(te_gmg *g, int enable);
/* name[i] (<=63 chars), calls[i], total_ms[i] (HIP events on the solver stream), cells[i]
 * (lattice sites the launches processed); returns number of rows written (<= max_rows) */
int te_gmg_profile_rows(te_gmg *g, int max_rows, char (*name)[64], int64_t *calls, double *total_ms,
                        int64_t *cells);
int te_gmg_profile_reset(te_gmg *g);
/* time only the launches of kernel class `name` (a row name of te_gmg_profile_rows); NULL or "" = every class.
 * A HIP event pair around a launch costs a few microseconds of stream time, which matters for a V-cycle of
 * a dozen launches: bench.py times only the dominant class inside its timed region. */
int te_gmg_profile_select(te_gmg *g, const char *name);
/* ... and only every `stride`-th launch of a timed class carries its event pair (stride <= 1: every launch). On this runtime an
 * event pair on a dispatch costs microseconds of stream time (profiles/r06_event_cost.txt: 24-28 us of a 210-us 4096^2 cycle with six
 * timed launches per cycle, 0-20 us of a 512^3 cycle with one): bench.py times every fourth launch of the dominant class inside its timed region; calls / cells / total_ms of
 * te_gmg_profile_rows count the timed launches only, so averages stay what they were. */
int te_gmg_profile_stride(te_gmg *g, int stride);

/* Where te_gmg_create spent its time -- the "GMG Setup" timer of apps/3d/steady.cpp:480-484 around GMG/CycleFactory3d.cpp:69-134,
 * broken down (milliseconds, host clock): out[0] device selection, context, streams, events (the first solver of a process also pays
 * the HIP runtime's start and the load of this library's code object here); out[1] the level tables, plans and transform matrices
 * built on the host; out[2] device allocations (hipMalloc), out[3] their number; out[4] uploads of the tables (hipMemcpy);
 * out[5] the work vectors of every level (allocation + zero fill queued); out[6] the final synchronisation; out[7] the whole call.
 * n <= 8 values are written; returns TE_OK. */
int te_gmg_setup_ms(const te_gmg *g, double *out, int n);

#ifdef __cplusplus
}
#endif
#endif
