// Everything the solver decides about one level before it touches the device: the face exchange plan, the stencil tables, the
// patch-solve plans, the transfers to the coarser level and the flags that choose between kernels. Host C++ only (no device
// header, nothing of te_gmg): gmg_core's buildLevel places the result on the device, tests/level_tables_check.cpp checks it
// for every rank of a partition in one process.
#pragma once
#include "mesh.hpp"
#include <cstddef>
#include <cstdint>
#include <vector>

namespace tei
{
// one exchange = for every peer: send [send_off, +send_cnt) and receive [recv_off, +recv_cnt) doubles
struct ExPlan {
	std::vector<int32_t> peers;
	std::vector<int64_t> send_off, send_cnt, recv_off, recv_cnt;
	bool empty() const { return peers.empty(); }
};

// the switches that shape the tables (TE_2D_SIMPLE, TE_NO_CFP, TE_2D_NO_MR_FUSE)
struct LevelBuildOpts {
	bool simple_2d = false, no_cfp = false, no_mr_fuse_2d = false;
};

// The members carry the names and meanings of the LevelHost members they become (gmg_internal.hpp); a vector that stays empty
// is a table the level does not have.
struct LevelTables {
	int    dim = 3, n = 0, P = 0, P_global = 0;
	bool   replicated = false, gathered = false;
	size_t nc = 0, nf = 0;
	// remote same-level faces
	ExPlan               fx;
	int                  nremote = 0;
	std::vector<int32_t> send_faces, f6off;
	// stencil
	std::vector<int32_t> face_kind, face_kind_patch, face_src, cf_desc, cf_slots, order, node_ids;
	std::vector<double>  face_kadj, rh2, cellvol, patch_vol, geom_starts, geom_h;
	int                  nslots = 0, ncf = 0, n_int = 0, n_bnd = 0;
	bool                 lds2d = false, fuse2d = false, fuse2_ok = false;
	// patch solve
	std::vector<int32_t> plan, zero_mode, psitab, ps_list, ps2_list;
	std::vector<double>  mats, lam, matsT, matfrag, matsym, psinv, mat2sym;
	bool                 sym_ok = false;
	int                  n_pure = 0, n_pure2 = 0;
	// transfers to the coarser level (coarser: there is one)
	bool                 coarser = false;
	int                  Pc = 0, n_up = 0, n_down = 0;
	std::vector<int32_t> parent, orth, child, copy, up_desc, down_desc, bc_desc, slot_parent, slot_orth;
	std::vector<int64_t> up_off, down_off, cbase;
	int64_t              up_total = 0, down_total = 0; // doubles in upbuf / downbuf
	ExPlan               tx_up, tx_down, tx_direct;
	// The same blocks in the same order with FACE-vector sizes (the restriction of a face vector to parents on other ranks,
	// te_faces_restrict / te_gmg_set_coefficient): an orthant block is the face vector of a patch of n/2 cells per axis,
	// faceDoubles(dim, n / 2) doubles, a copy-through block the patch's own faceDoubles(dim, n). up_foff[i] / down_foff[i]: where
	// block i of up_desc / down_desc starts in the face send / receive buffer; tx_fup: children send, parents receive (under
	// repl_up one copy to everybody, as tx_up). Nothing travels down: there is no prolongation of a face vector.
	std::vector<int64_t> up_foff, down_foff;
	int64_t              up_ftotal = 0, down_ftotal = 0;
	ExPlan               tx_fup;
	bool prolong_fusable = false, prolong_fusable_cf = false, has_copy = false, repl_up = false, repl_direct = false,
	     post_exchange_free = false;
	// interfaces (mesh.hpp Level::iface_*), passed through
	int                  nif = -1;
	std::vector<int32_t> if_own, if_start, if_contrib;
	// physical faces (mesh.hpp bfaceIndex), passed through
	int                  nbf = 0;
	std::vector<int32_t> bface;
	// te_boundary_restrict (single rank, a coarser level exists): one row of 5 per physical face of the COARSER level, in its
	// boundary-vector order: [0] 1 = a patch that copies through ([1] = its block on this level), 0 = the mean of the blocks
	// [1 + q] of the children, q = the child's orthant bits on the face's remaining axes (the lower axis in bit 0)
	std::vector<int32_t> brestrict;
};

/// doubles of a face vector per patch of m cells per axis: dim lower-face blocks of m^dim and dim upper-face blocks of m^(dim-1)
inline int64_t faceDoubles(int dim, int64_t m) { return dim == 3 ? 3 * m * m * m + 3 * m * m : 2 * m * m + 2 * m; }

/// fills `out` for level li of H as rank H.rank sees it; TE_OK, or an error code with te::fail's message
int computeLevelTables(const te::Hierarchy &H, int li, const LevelBuildOpts &o, LevelTables &out);

} // namespace tei
