// Host-side mesh model for the MI355X GMG path: octree/quadtree, per-level patch
// extraction, static Morton partition, and the flattened SoA tables the HIP kernels read.
//
// Replaces (behaviour, not code) the reference's
//   Tree<D>            src/Thunderegg/OctTree.h:34-213  (file reader, refineLeaves)
//   Node<D>            src/Thunderegg/OctNode.h:30-130
//   extractLevel       src/Thunderegg/ThundereggDomGen.h:127-222 (which nodes form a level,
//                      Normal / Coarse / Fine neighbour classification, parent + orthant)
//   level truncation   src/Thunderegg/GMG/CycleFactory3d.cpp:101-104 (max_levels,
//                      patches_per_proc)
//   PatchInfo<D>       src/Thunderegg/PatchInfo.h:74-277 (only the fields kernels consume)
// The Zoltan hypergraph partitioner (ThundereggDomGen.h:223-648) is replaced by a
// deterministic Morton-range partition: one contiguous Morton range of finest-level patches
// per rank; a coarser patch lives where its orthant-0 child (or itself, if it does not
// coarsen) lives.
#pragma once
#include <cstdint>
#include <map>
#include <string>
#include <vector>

namespace te
{
constexpr int MAX_D    = 3;
constexpr int MAX_SIDE = 6;
constexpr int MAX_ORTH = 8;

/// Side numbering follows src/Thunderegg/Side.h:51-56: W,E,S,N,B,T = 0..5; axis = side/2.
/// Orthant numbering follows Side.h:183-211: bit0 = x upper, bit1 = y upper, bit2 = z upper.
struct Node {
	int    id     = -1;
	int    level  = -1;
	int    parent = -1;
	double lengths[MAX_D];
	double starts[MAX_D];
	int    nbr[MAX_SIDE];
	int    child[MAX_ORTH];
	Node();
	bool hasChildren() const { return child[0] != -1; }
};

struct Tree {
	int                 dim = 3;
	std::map<int, Node> nodes;
	int                 root       = 0;
	int                 num_levels = 0;
	int                 max_id     = 0;
	/// depth of the root as stored in the file (shipped files use level = 1)
	int root_level = 1;

	static Tree read(const std::string &path, int dim);
	/// single root node on the unit box, level 1 (what a 1-node mesh file holds)
	static Tree unitRoot(int dim);
	/// the same on the box [starts, starts + lengths): the auxiliary tree of the sub-patch coarse solve (gmg_coefcoarse.hip); no
	/// public mesh call makes one
	static Tree boxRoot(int dim, const double *starts, const double *lengths);
	/// split every leaf once; new ids are ++max_id in (depth, id) leaf order then orthant
	/// order, as OctTree.h:119-179 + :183-189 assign them.
	void refineLeaves();
	void refineNode(int id);
	int  depthOf(int id) const;
	/// ids of the leaves, ascending
	std::vector<int> leaves() const;
	/// face-balanced: two leaves that share a face differ by at most one level (faces are all the solver reads)
	bool isBalanced() const;
	/// A new tree from per-leaf flags (+1 refine, 0 keep, -1 coarsen; leaves not named: 0); *this is untouched. The rule is stated
	/// in include/te_hip.h (te_mesh_adapt). Throws std::runtime_error for an unknown id, a non-leaf, a duplicate or another flag value.
	/// The reference has refineNode (OctTree.h:180) only: no balance, no coarsening.
	Tree adapt(int count, const int32_t *ids, const int32_t *flags) const;
};

enum NbrKind : int32_t { NBR_NONE = 0, NBR_NORMAL = 1, NBR_COARSE = 2, NBR_FINE = 3 };

/// One multigrid level as seen by ONE rank. "Global" arrays cover every patch of the level
/// (small: tens of bytes per patch); local arrays cover this rank's patches only.
struct Level {
	int dim = 3;
	int n   = 0; ///< cells per axis per patch (cubic patches, as the reference's solvers assume)
	int tree_level = 0;

	// ---- global (all ranks' patches), Morton order ------------------------------------
	int                  P_global = 0;
	std::vector<int32_t> g_id;    ///< tree node id
	std::vector<int32_t> g_rank;  ///< owner rank
	std::vector<int32_t> g_local; ///< index inside the owner's local numbering
	std::vector<double>  g_starts;  ///< [P][dim]
	std::vector<double>  g_lengths; ///< [P][dim]
	std::vector<int32_t> g_nbr_kind; ///< [P][2*dim]
	std::vector<int32_t> g_nbr;      ///< [P][2*dim][4] global patch indices, -1 unused
	std::vector<int32_t> g_nbr_orth; ///< [P][2*dim] quadrant on the coarse nbr face (kind COARSE)
	std::vector<int32_t> g_parent;   ///< [P] global patch index in the next coarser level (-1 none)
	std::vector<int32_t> g_orth_on_parent; ///< [P] 0..2^dim-1, or -1 = copies through

	// ---- local --------------------------------------------------------------------------
	int                  P = 0;   ///< patches owned by this rank
	/// every rank holds (and computes) the whole level: g_rank is this rank's number for every patch, P == P_global
	bool                 replicated = false;
	std::vector<int32_t> l2g;     ///< [P] local -> global index

	// ---- interfaces (single-rank hierarchies only; num_ifaces = -1 on a sharded one) --------------------------------
	/// The interface unknowns of the Schur-complement route: one block of n^(dim-1) values per interface, numbered in
	/// first-seen order over the patches and their sides as SchurHelper<D>::indexDomainIfacesLocal does (SchurHelper.h:
	/// 377-397; ids SchurInfo.h:141-150 normal, :229-237 coarse, :322-331 fine).
	int                  num_ifaces = -1;
	std::vector<int32_t> iface_own;   ///< [P][2*dim] the interface patch p sees on side s, -1 on a physical face
	/// what interpolateToInterface (SchurHelper.h:333-343) sums into each interface: the contributions of interface i are
	/// iface_contrib[iface_start[i] .. iface_start[i+1]), each (patch, side, IfaceKind, quadrant), in (patch, side) order
	std::vector<int32_t> iface_start;   ///< [num_ifaces + 1]
	std::vector<int32_t> iface_contrib; ///< [..][4]
};

/// the five IfaceType cases of TriLinInterp / BilinearInterpolator, seen from the contributing patch's side
enum IfaceKind : int32_t {
	IF_NORMAL = 0,          ///< same-level neighbour: 1/2 of the own face layer
	IF_FINE_TO_FINE = 1,    ///< this patch is the fine side, its own interface
	IF_FINE_TO_COARSE = 2,  ///< this patch is the fine side, the coarse neighbour's interface (quadrant = its position there)
	IF_COARSE_TO_COARSE = 3,///< this patch is the coarse side, its own interface
	IF_COARSE_TO_FINE = 4   ///< this patch is the coarse side, fine neighbour `quadrant`'s interface
};

/// Where the levels with few patches live when nranks > 1 (the patches_per_proc idea of CycleFactory3d.cpp:104 without
/// cutting the hierarchy): a level with fewer than `agglomerate` patches per rank -- and at most `agglomerate_max` patches
/// in total -- and every level below it is gathered: on every rank (`replicate`, 3D) or on rank 0. Negative = the default
/// (64 / 64 / 1), which the environment may override (TE_AGGLOMERATE, TE_AGGLOMERATE_MAX, TE_REPLICATE: read by
/// te_hier_build only, once per call, and recorded in the hierarchy).
struct Placement {
	double agglomerate     = -1.0;
	int    agglomerate_max = -1, replicate = -1;
};

struct Hierarchy {
	int                dim = 3;
	int                n   = 0;
	int                rank = 0, nranks = 1;
	bool               neumann = false; ///< every side of the domain is Neumann (the constant null space)
	/// bit s = the domain's side s (W,E,S,N,B,T) is a Neumann boundary, the others Dirichlet: one kind per side of the DOMAIN
	int                neumann_sides = 0;
	std::vector<Level> levels; ///< [0] = finest
	/// placement of the small levels over the ranks (see Placement), as this hierarchy was built: part of what every rank
	/// must agree on (te_gmg checks it across the ranks before the first cycle)
	double agglomerate = 64.0;
	int    agglomerate_max = 64, replicate = 1;
	/// Level 0 holds exactly the tree's leaves. Per level-0 patch (global order): its tree node id, the id of its parent IN THE TREE
	/// (-1: the root) and its orthant there (-1: the root) -- what a transfer between two meshes needs (te_vec_regrid). Host only.
	std::vector<int32_t> leaf_id, leaf_parent, leaf_orth;

	/// Build every level the reference's CycleFactory would build
	/// (CycleFactory3d.cpp:69-134): finest first, then coarser tree levels while
	/// (max_levels <= 0 || built < max_levels) and patches/nranks >= patches_per_proc.
	static Hierarchy build(const Tree &t, int n, bool neumann, int max_levels,
	                       double patches_per_proc, int rank, int nranks, const Placement &pl = Placement());
	/// the same with a kind per side; throws for a bit at or above 2 dim
	static Hierarchy buildSides(const Tree &t, int n, int neumann_sides, int max_levels,
	                            double patches_per_proc, int rank, int nranks, const Placement &pl = Placement());
};

/// This rank's physical faces of `lv` (no neighbour: NBR_NONE), numbered in (patch, side) order over its local patches:
/// idx[P][2 dim] = the face's number, -1 on a face with a neighbour; returns how many there are. A level that lives on every
/// rank is numbered whole on every rank.
int bfaceIndex(const Level &lv, std::vector<int32_t> &idx);

/// fills the interface tables of `lv` (all patches of the level, global order)
void buildIfaces(Level &lv);

uint64_t mortonKey(const double *starts, const double *root_starts, const double *root_lengths,
                   int dim, int bits);
} // namespace te
