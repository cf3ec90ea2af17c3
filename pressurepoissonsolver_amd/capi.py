"""ctypes binding of include/te_hip.h (libte_hip.so) — plumbing only.

The shared library is the product; this module adds nothing numerical. It fails loudly when the
library is missing (`TeLibraryMissing`): there is no Python / torch / CPU fallback for any
operation.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# (TE_HIP_LIB_PATH: tooling -- another build of the library, build.build_variant, for same-box A/B runs)
LIB_PATH = os.environ.get("TE_HIP_LIB_PATH") or os.path.join(_HERE, "libte_hip.so")


class TeError(RuntimeError):
    """Non-zero status from the C ABI (the reference's convention is `throw 3;`)."""

    def __init__(self, code, msg):
        super().__init__(f"te_hip error {code}: {msg}")
        self.code = code


class TeLibraryMissing(ImportError):
    pass


TE_OK, TE_EINVAL, TE_EHIP, TE_ESTATE, TE_EIO, TE_EUNSUPPORTED, TE_ENOMEM = 0, -1, -2, -3, -4, -5, -6
SMOOTH_PATCH_SOLVE, SMOOTH_JACOBI, SMOOTH_RBGS, SMOOTH_PATCH_BCGS = 0, 1, 2, 3
PROBLEM_TRIG, PROBLEM_GAUSS, PROBLEM_RANDOM = 0, 1, 2
SCHUR_PREC_NONE, SCHUR_PREC_CHEB = 0, 1
INTERP_DIRECT, INTERP_LINEAR = 0, 1  # TE_INTERP_*: DrctIntp (the default), tri-/bilinear
SLABS_STENCIL, SLABS_SWEEP = 0, 1  # TE_SLABS_*: which slab rule te_gmg_slab_count reports
FACE_MEAN, FACE_HARMONIC, FACE_RECIP_MEAN = 0, 1, 2  # TE_FACE_*: how te_faces_from_cells combines the two operands of a face
SLOPE_ZERO, SLOPE_MINMOD, SLOPE_MC, SLOPE_CENTRAL = 0, 1, 2, 3  # TE_SLOPE_*: the slope kinds of te_cell_slopes / te_advect_muscl
COEF_COARSE_SWEEPS, COEF_COARSE_SUBCYCLE = 0, 1  # TE_COEF_COARSE_*: the coarsest level of the cycle with a coefficient


class CycleOpts(C.Structure):
    """GMG/CycleOpts.h:51-79 + the smoother selection of this build."""

    _fields_ = [("pre_sweeps", C.c_int32), ("post_sweeps", C.c_int32), ("coarse_sweeps", C.c_int32),
                ("mid_sweeps", C.c_int32), ("cycle_type", C.c_int32), ("smoother", C.c_int32),
                ("omega", C.c_double), ("exact_coarse", C.c_int32), ("fuse", C.c_int32)]


EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                          C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                          C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_void_p)

ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int, C.c_int)

# every symbol include/te_hip.h declares: (restype, argtypes)
_P = C.c_void_p
_D = C.c_double
_I = C.c_int
_PI32 = C.POINTER(C.c_int32)
_PD = C.POINTER(C.c_double)
SYMBOLS = {
    "te_last_error": (C.c_char_p, []),
    "te_version": (C.c_char_p, []),
    "te_mesh_read": (_I, [C.c_char_p, _I, C.POINTER(_P)]),
    "te_mesh_unit_root": (_I, [_I, C.POINTER(_P)]),
    "te_mesh_refine_leaves": (_I, [_P]),
    "te_mesh_num_nodes": (_I, [_P]),
    "te_mesh_num_levels": (_I, [_P]),
    "te_mesh_dim": (_I, [_P]),
    "te_mesh_get_nodes": (_I, [_P, _P, _P, _P, _P, _P]),
    "te_mesh_num_leaves": (_I, [_P]),
    "te_mesh_leaves": (_I, [_P, _P]),
    "te_mesh_is_balanced": (_I, [_P]),
    "te_mesh_adapt": (_I, [_P, _I, _P, _P, C.POINTER(_P)]),
    "te_mesh_destroy": (None, [_P]),
    "te_hier_build": (_I, [_P, _I, _I, _I, _D, _I, _I, C.POINTER(_P)]),
    "te_hier_build_placed": (_I, [_P, _I, _I, _I, _D, _I, _I, _D, _I, _I, C.POINTER(_P)]),
    "te_hier_build_bc": (_I, [_P, _I, _I, _I, _D, _I, _I, _D, _I, _I, C.POINTER(_P)]),
    "te_hier_neumann_sides": (_I, [_P]),
    "te_hier_singular": (_I, [_P]),
    "te_hier_num_bfaces": (_I, [_P, _I, C.POINTER(_I)]),
    "te_hier_bface_index": (_I, [_P, _I, _P]),
    "te_hier_placement": (_I, [_P, _PD, C.POINTER(_I), C.POINTER(_I)]),
    "te_hier_num_levels": (_I, [_P]),
    "te_hier_dim": (_I, [_P]),
    "te_hier_n": (_I, [_P]),
    "te_hier_level_sizes": (_I, [_P, _I, C.POINTER(_I), C.POINTER(_I)]),
    "te_hier_level_replicated": (_I, [_P, _I]),
    "te_hier_level_tables": (_I, [_P, _I] + [_P] * 10),
    "te_hier_level_l2g": (_I, [_P, _I, _P]),
    "te_hier_leaf_tree": (_I, [_P, _P, _P, _P]),
    "te_hier_num_ifaces": (_I, [_P, _I, C.POINTER(_I)]),
    "te_hier_iface_index": (_I, [_P, _I, _P]),
    "te_hier_destroy": (None, [_P]),
    "te_cycle_opts_default": (None, [C.POINTER(CycleOpts)]),
    "te_gmg_create": (_I, [_P, _I, C.POINTER(_P)]),
    "te_gmg_destroy": (None, [_P]),
    "te_gmg_num_levels": (_I, [_P]),
    "te_gmg_sync": (_I, [_P]),
    "te_gmg_stream": (_P, [_P]),
    "te_vec_create": (_I, [_P, _I, C.POINTER(_P)]),
    "te_vec_create_iface": (_I, [_P, _I, C.POINTER(_P)]),
    "te_vec_create_boundary": (_I, [_P, _I, C.POINTER(_P)]),
    "te_vec_create_faces": (_I, [_P, _I, C.POINTER(_P)]),
    "te_vec_destroy": (None, [_P]),
    "te_vec_size": (C.c_size_t, [_P]),
    "te_vec_upload": (_I, [_P, _P]),
    "te_vec_download": (_I, [_P, _P]),
    "te_vec_upload_patches": (_I, [_P, _I, _I, _P]),
    "te_vec_download_patches": (_I, [_P, _I, _I, _P]),
    "te_vec_device_ptr": (_P, [_P]),
    "te_vec_set": (_I, [_P, _D]),
    "te_vec_scale": (_I, [_P, _D]),
    "te_vec_shift": (_I, [_P, _D]),
    "te_vec_copy": (_I, [_P, _P]),
    "te_vec_add": (_I, [_P, _P]),
    "te_vec_add_scaled": (_I, [_P, _D, _P]),
    "te_vec_add_scaled2": (_I, [_P, _D, _P, _D, _P]),
    "te_vec_scale_then_add": (_I, [_P, _D, _P]),
    "te_vec_scale_then_add_scaled": (_I, [_P, _D, _D, _P]),
    "te_vec_scale_then_add_scaled2": (_I, [_P, _D, _D, _P, _D, _P]),
    "te_vec_multiply": (_I, [_P, _P]),
    "te_vec_two_norm_sq": (_I, [_P, _PD]),
    "te_vec_inf_norm": (_I, [_P, _PD]),
    "te_vec_dot": (_I, [_P, _P, _PD]),
    "te_vec_checksum": (_I, [_P, C.POINTER(C.c_uint64)]),
    "te_apply": (_I, [_P, _I, _P, _P]),
    "te_patch_apply": (_I, [_P, _I, _P, _P]),
    "te_residual": (_I, [_P, _I, _P, _P, _P]),
    "te_residual_norm_sq": (_I, [_P, _I, _P, _P, _P, _PD]),
    "te_smooth": (_I, [_P, _I, _P, _P, _I, _D, _I]),
    "te_restrict": (_I, [_P, _I, _P, _P]),
    "te_prolong_add": (_I, [_P, _I, _P, _P]),
    "te_prolong_linear_add": (_I, [_P, _I, _P, _P]),
    "te_prolong_quadratic": (_I, [_P, _I, _P, _P]),
    "te_boundary_restrict": (_I, [_P, _I, _P, _P]),
    "te_fmg": (_I, [_P, _P, _P, _P, _P, _I, _PD]),
    "te_patch_indicator": (_I, [_P, _I, _P, _P]),
    "te_vec_regrid": (_I, [_P, _P, _P, _P]),
    "te_faces_regrid": (_I, [_P, _P, _P, _P]),
    "te_gmg_set_interpolator": (_I, [_P, _I]),
    "te_gmg_interpolator": (_I, [_P]),
    "te_vcycle": (_I, [_P, C.POINTER(CycleOpts), _P, _P]),
    "te_bicgstab": (_I, [_P, C.POINTER(CycleOpts), _P, _P, _I, _D, C.POINTER(_I), _PD]),
    "te_gmg_release_workspace": (_I, [_P]),
    "te_gmg_set_option": (_I, [_P, C.c_char_p, C.c_char_p]),
    "te_gmg_slab_count": (_I, [_P, _I, _I, _P]),
    "te_gmg_set_exchange": (_I, [_P, EXCHANGE_FN, _P]),
    "te_rccl_unique_id": (_I, [C.c_char_p, C.c_char_p]),
    "te_gmg_use_rccl": (_I, [_P, C.c_char_p, C.c_char_p, _I, _I]),
    "te_gmg_set_allreduce": (_I, [_P, ALLREDUCE_FN, _P]),
    "te_gmg_verify_schedule": (_I, [_P, C.POINTER(CycleOpts)]),
    "te_gmg_autotune": (_I, [_P, C.POINTER(CycleOpts), _I, _PD, C.c_char_p, _I]),
    "te_gmg_comm_info": (_I, [_P, C.POINTER(_I), C.POINTER(_I)]),
    "te_gmg_use_push": (_I, [_P, _I]),
    "te_gmg_push_failed": (_I, [_P]),
    "te_gmg_set_patch_bcgs": (_I, [_P, _D, _I]),
    "te_gmg_patch_bcgs_iterations": (_I, [_P, _I, _P]),
    "te_gmg_exchange_selftest": (_I, [_P, _I]),
    "te_gmg_watchdog_selftest": (_I, [_P, _D]),
    "te_gmg_setup_ms": (_I, [_P, _PD, _I]),
    "te_gmg_profile": (_I, [_P, _I]),
    "te_gmg_profile_rows": (_I, [_P, _I, _P, _P, _P, _P]),
    "te_gmg_profile_reset": (_I, [_P]),
    "te_gmg_profile_select": (_I, [_P, C.c_char_p]),
    "te_gmg_profile_stride": (_I, [_P, _I]),
    "te_init_problem": (_I, [_P, _I, _I, _I, _P, _P]),
    "te_add_boundary_rhs": (_I, [_P, _I, _P, _P]),
    "te_boundary_sample": (_I, [_P, _I, _I, _P]),
    "te_init_problem_sides": (_I, [_P, _I, _I, _P, _P]),
    "te_iface_interp": (_I, [_P, _I, _P, _P]),
    "te_apply_with_interface": (_I, [_P, _I, _P, _P, _P]),
    "te_add_iface_rhs": (_I, [_P, _I, _P, _P]),
    "te_solve_with_interface": (_I, [_P, _I, _P, _P, _P, _P]),
    "te_schur_apply": (_I, [_P, _I, _P, _P]),
    "te_schur_cheb": (_I, [_P, _I, _P, _P]),
    "te_schur_solve": (_I, [_P, _I, _I, _P, _P, _P, _I, _D, C.POINTER(_I), _PD]),
    "te_gradient": (_I, [_P, _I, _P, _P, _P]),
    "te_divergence": (_I, [_P, _I, _D, _P, _P]),
    "te_project": (_I, [_P, _I, _D, _P, _P, _P]),
    "te_faces_from_cells": (_I, [_P, _I, _I, _P, _P, _P]),
    "te_project_weighted": (_I, [_P, _I, _D, _P, _P, _P, _P]),
    "te_add_boundary_rhs_weighted": (_I, [_P, _I, _P, _P, _P]),
    "te_advect_flux": (_I, [_P, _I, _P, _P, _P, _P]),
    "te_advect": (_I, [_P, _I, _D, _P, _P, _P, _P]),
    "te_faces_match": (_I, [_P, _I, _P]),
    "te_faces_max_rate": (_I, [_P, _I, _P, _PD]),
    "te_cell_slopes": (_I, [_P, _I, _I, _P, _P, _P, _P, _P]),
    "te_advect_flux_muscl": (_I, [_P, _I, _I, _P, _P, _P, _P]),
    "te_advect_muscl": (_I, [_P, _I, _D, _I, _P, _P, _P, _P]),
    "te_faces_restrict": (_I, [_P, _I, _P, _P]),
    "te_gmg_set_coefficient": (_I, [_P, _P]),
    "te_gmg_has_coefficient": (_I, [_P]),
    "te_gmg_coefficient": (_I, [_P, _I, _P]),
    "te_gmg_set_reaction": (_I, [_P, _P]),
    "te_gmg_has_reaction": (_I, [_P]),
    "te_gmg_reaction": (_I, [_P, _I, _P]),
    "te_gmg_set_coef_coarse": (_I, [_P, _I, _I, _I]),
    "te_gmg_coef_coarse": (_I, [_P, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I)]),
    "te_integrate": (_I, [_P, _I, _P, _P]),
    "te_volume": (_I, [_P, _I, _P]),
}

_lib = None


def lib():
    """Load libte_hip.so (once). Raises TeLibraryMissing if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise TeLibraryMissing(
                f"{LIB_PATH} not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). There is no fallback implementation.")
        # One HIP runtime per process: PyTorch's ROCm wheel bundles its own libamdhip64.so.7 (same soname as
        # /opt/rocm's). If torch is loaded first the dynamic loader hands that copy to libte_hip.so as well;
        # the other order leaves two runtimes that cannot see each other's allocations (torch.distributed /
        # RCCL would then reject our device pointers). A pure C++ host simply gets /opt/rocm's runtime.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc):
    if rc != TE_OK:
        raise TeError(rc, lib().te_last_error().decode())


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Mesh:
    """Tree<D> (src/Thunderegg/OctTree.h:34)."""

    def __init__(self, handle):
        self.h = handle

    @classmethod
    def read(cls, path, dim=3):
        h = C.c_void_p()
        check(lib().te_mesh_read(os.fsencode(path), dim, C.byref(h)))
        return cls(h)

    @classmethod
    def unit_root(cls, dim=3):
        h = C.c_void_p()
        check(lib().te_mesh_unit_root(dim, C.byref(h)))
        return cls(h)

    @classmethod
    def uniform(cls, dim, divides):
        """1-node tree refined `divides` times: 2^(dim*divides) leaves."""
        m = cls.unit_root(dim)
        for _ in range(divides):
            m.refine_leaves()
        return m

    def refine_leaves(self):
        check(lib().te_mesh_refine_leaves(self.h))

    @property
    def dim(self):
        return lib().te_mesh_dim(self.h)

    @property
    def num_nodes(self):
        return lib().te_mesh_num_nodes(self.h)

    @property
    def num_levels(self):
        return lib().te_mesh_num_levels(self.h)

    def nodes(self):
        n, d = self.num_nodes, self.dim
        out = dict(ilp=np.zeros((n, 3), np.int32), lengths=np.zeros((n, d)), starts=np.zeros((n, d)),
                   nbr=np.zeros((n, 2 * d), np.int32), child=np.zeros((n, 1 << d), np.int32))
        check(lib().te_mesh_get_nodes(self.h, _ptr(out["ilp"]), _ptr(out["lengths"]), _ptr(out["starts"]),
                                      _ptr(out["nbr"]), _ptr(out["child"])))
        return out

    def leaves(self):
        """ids of the leaves, ascending (level 0 of every hierarchy built from this mesh holds exactly these)"""
        n = lib().te_mesh_num_leaves(self.h)
        if n < 0:
            check(n)
        out = np.zeros(n, np.int32)
        check(lib().te_mesh_leaves(self.h, _ptr(out)))
        return out

    def is_balanced(self):
        """face-balanced: two leaves that share a face differ by at most one level"""
        r = lib().te_mesh_is_balanced(self.h)
        if r < 0:
            check(r)
        return bool(r)

    def adapt(self, flags):
        """te_mesh_adapt: a NEW mesh from {leaf id: +1 refine / 0 keep / -1 coarsen} (leaves not named: 0); self is untouched"""
        ids = np.array(list(flags.keys()), np.int32)
        fl = np.array([flags[k] for k in flags], np.int32)
        h = C.c_void_p()
        check(lib().te_mesh_adapt(self.h, len(ids), _ptr(ids), _ptr(fl), C.byref(h)))
        return Mesh(h)

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.te_mesh_destroy(self.h)
            self.h = None


SIDES = ("west", "east", "south", "north", "bottom", "top")  # s = 2 * axis + upper (Side.h:51-56)


def sides_mask(names):
    """the bit mask of an iterable of side names"""
    mask = 0
    for s in names:
        mask |= 1 << SIDES.index(s)
    return mask


class Hierarchy:
    """DomainGenerator + the CycleFactory level loop (ThundereggDomGen.h, CycleFactory3d.cpp:98-127)."""

    def __init__(self, mesh, n, neumann=False, max_levels=0, patches_per_proc=0.0, rank=0, nranks=1, placement=None, neumann_sides=None):
        """placement = (agglomerate, agglomerate_max, replicate) spelled out (a negative entry = the default), or None: the
        environment's TE_AGGLOMERATE / TE_AGGLOMERATE_MAX / TE_REPLICATE, read once by te_hier_build.
        neumann_sides: one boundary kind per side of the domain (te_hier_build_bc) -- an int mask (bit 2 * axis + upper) or an
        iterable of side names ("west", "east", "south", "north", "bottom", "top"); the other sides are Dirichlet"""
        self.h = C.c_void_p()
        if neumann_sides is not None:
            if neumann:
                raise ValueError("Hierarchy: give neumann or neumann_sides, not both")
            mask = neumann_sides if isinstance(neumann_sides, (int, np.integer)) else sides_mask(neumann_sides)
            if placement is None:  # (the environment's placement, as te_hier_build reads it)
                e = os.environ.get
                placement = (float(e("TE_AGGLOMERATE", -1.0)), int(e("TE_AGGLOMERATE_MAX", -1)),
                             int(int(e("TE_REPLICATE")) != 0) if e("TE_REPLICATE") is not None else -1)
            agg, cap, rep = placement
            check(lib().te_hier_build_bc(mesh.h, n, int(mask), max_levels, float(patches_per_proc), rank, nranks,
                                         float(agg), int(cap), int(rep), C.byref(self.h)))
        elif placement is None:
            check(lib().te_hier_build(mesh.h, n, int(neumann), max_levels, float(patches_per_proc), rank, nranks,
                                      C.byref(self.h)))
        else:
            agg, cap, rep = placement
            check(lib().te_hier_build_placed(mesh.h, n, int(neumann), max_levels, float(patches_per_proc), rank, nranks,
                                             float(agg), int(cap), int(rep), C.byref(self.h)))
        self.n = n
        self.neumann_sides = lib().te_hier_neumann_sides(self.h)
        self.singular = bool(lib().te_hier_singular(self.h))
        self.neumann = self.singular  # (true only when EVERY side is Neumann)
        self.dim = lib().te_hier_dim(self.h)
        self.num_levels = lib().te_hier_num_levels(self.h)
        self.rank, self.nranks = rank, nranks

    def sizes(self, level):
        a, b = C.c_int(), C.c_int()
        check(lib().te_hier_level_sizes(self.h, level, C.byref(a), C.byref(b)))
        return a.value, b.value

    def placement(self):
        """(agglomerate, agglomerate_max, replicate) this hierarchy was built with"""
        a, b, c = C.c_double(), C.c_int(), C.c_int()
        check(lib().te_hier_placement(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def replicated(self, level):
        """the level lives on every rank (a gathered coarse level, TE_REPLICATE): each rank holds and computes all of it"""
        r = lib().te_hier_level_replicated(self.h, level)
        if r < 0:
            check(r)
        return bool(r)

    def tables(self, level):
        P = self.sizes(level)[1]
        d, ns = self.dim, 2 * self.dim
        t = dict(id=np.zeros(P, np.int32), rank=np.zeros(P, np.int32), local=np.zeros(P, np.int32),
                 starts=np.zeros((P, d)), lengths=np.zeros((P, d)), nbr_kind=np.zeros((P, ns), np.int32),
                 nbr=np.zeros((P, ns, 4), np.int32), nbr_orth=np.zeros((P, ns), np.int32),
                 parent=np.zeros(P, np.int32), orth_on_parent=np.zeros(P, np.int32))
        check(lib().te_hier_level_tables(self.h, level, *[_ptr(t[k]) for k in (
            "id", "rank", "local", "starts", "lengths", "nbr_kind", "nbr", "nbr_orth", "parent",
            "orth_on_parent")]))
        return t

    def leaf_tree(self):
        """where the level-0 patches (= the mesh's leaves) sit in the tree, global order: dict(id, tree_parent, orthant)"""
        P = self.sizes(0)[1]
        t = dict(id=np.zeros(P, np.int32), tree_parent=np.zeros(P, np.int32), orthant=np.zeros(P, np.int32))
        check(lib().te_hier_leaf_tree(self.h, _ptr(t["id"]), _ptr(t["tree_parent"]), _ptr(t["orthant"])))
        return t

    def num_ifaces(self, level=0):
        """interfaces of the level (SchurHelper.h:377-397); single-rank hierarchies only"""
        out = C.c_int()
        check(lib().te_hier_num_ifaces(self.h, level, C.byref(out)))
        return out.value

    def iface_index(self, level=0):
        """[P][2*dim] the interface patch p sees on side s, -1 on a physical face"""
        out = np.zeros((self.sizes(level)[1], 2 * self.dim), np.int32)
        check(lib().te_hier_iface_index(self.h, level, _ptr(out)))
        return out

    def num_bfaces(self, level=0):
        """this rank's physical faces on the level: the blocks of a boundary vector"""
        out = C.c_int()
        check(lib().te_hier_num_bfaces(self.h, level, C.byref(out)))
        return out.value

    def bface_index(self, level=0):
        """[P_local][2*dim] the number of the physical face on side s of local patch p ((patch, side) order), -1 elsewhere"""
        out = np.zeros((self.sizes(level)[0], 2 * self.dim), np.int32)
        check(lib().te_hier_bface_index(self.h, level, _ptr(out)))
        return out

    def l2g(self, level):
        out = np.zeros(self.sizes(level)[0], np.int32)
        check(lib().te_hier_level_l2g(self.h, level, _ptr(out)))
        return out

    def cells(self, level):
        return self.sizes(level)[0] * self.n ** self.dim

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.te_hier_destroy(self.h)
            self.h = None


def regrid(src_g, u_src, dst_g, u_dst):
    """te_vec_regrid: u_dst (level 0 of dst_g) = u_src (level 0 of src_g) carried to dst_g's mesh, one te_mesh_adapt away:
    copy / quadratic refinement / AvgRstr coarsening per destination leaf"""
    check(lib().te_vec_regrid(src_g.h, u_src.h, dst_g.h, u_dst.h))


def regrid_faces(src_g, U_src, dst_g, U_dst):
    """te_faces_regrid: the face vector U_dst (level 0 of dst_g) = U_src (level 0 of src_g) carried to dst_g's mesh, one te_mesh_adapt
    away: copy / divergence-preserving second-order refinement / face averages per destination leaf"""
    check(lib().te_faces_regrid(src_g.h, U_src.h, dst_g.h, U_dst.h))


def face_vector_size(n, dim):
    """doubles per patch of a face vector (te_vec_create_faces)"""
    return dim * n ** dim + dim * n ** (dim - 1)


def face_vector_views(a, n, dim):
    """the host array of a face vector as (lo[P, dim, n..n], hi[P, dim, n^(dim-1)]): lo[p, a] = the components on the lower
    a-faces of patch p's cells (numpy index order z, y, x), hi[p, a] = those on the patch's upper a-face. Views: writing
    through them changes `a`."""
    a = np.asarray(a)
    per = a.reshape(-1, face_vector_size(n, dim))
    nlo = dim * n ** dim
    return per[:, :nlo].reshape((-1, dim) + (n,) * dim), per[:, nlo:].reshape((-1, dim, n ** (dim - 1)))


class Vec:
    """Vector<D> on the device (Vector.h:179-321); method names follow the reference."""

    def __init__(self, gmg, level=0, data=None, iface=False, boundary=False, faces=False):
        """iface: an interface vector of the level (SchurHelper::getNewSchurVec), one block of n^(dim-1) per interface;
        boundary: a boundary vector (te_vec_create_boundary), one such block per physical face;
        faces: a face vector (te_vec_create_faces), dim n^dim + dim n^(dim-1) doubles per patch"""
        self.gmg, self.level, self.iface = gmg, level, bool(iface or boundary)  # (iface: the blocks are faces, not patches)
        self.faces = bool(faces)
        self.h = C.c_void_p()
        create = lib().te_vec_create_boundary if boundary else (lib().te_vec_create_iface if iface else lib().te_vec_create)
        if faces:
            create = lib().te_vec_create_faces
        check(create(gmg.h, level, C.byref(self.h)))
        if data is not None:
            self.upload(data)

    @property
    def size(self):
        return lib().te_vec_size(self.h)

    def upload(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64).ravel()
        if a.size != self.size:
            raise ValueError(f"upload: {a.size} values for a vector of {self.size}")
        check(lib().te_vec_upload(self.h, _ptr(a)))

    def download(self):
        out = np.empty(self.size, np.float64)
        check(lib().te_vec_download(self.h, _ptr(out)))
        return out

    def _block(self):
        n, d = self.gmg.hier.n, self.gmg.hier.dim
        return face_vector_size(n, d) if getattr(self, "faces", False) else n ** (d - self.iface)

    def upload_patches(self, first, a):
        """Vector<D>::getLocalData(i) write path for a run of patches"""
        a = np.ascontiguousarray(a, dtype=np.float64)
        nc = self._block()
        if a.size % nc:
            raise ValueError("upload_patches: not a whole number of patches")
        check(lib().te_vec_upload_patches(self.h, first, a.size // nc, _ptr(a.ravel())))

    def download_patches(self, first, count):
        out = np.empty(count * self._block(), np.float64)
        check(lib().te_vec_download_patches(self.h, first, count, _ptr(out)))
        return out

    def device_ptr(self):
        return lib().te_vec_device_ptr(self.h)

    def set(self, alpha): check(lib().te_vec_set(self.h, alpha))
    def scale(self, alpha): check(lib().te_vec_scale(self.h, alpha))
    def shift(self, delta): check(lib().te_vec_shift(self.h, delta))
    def copy(self, b): check(lib().te_vec_copy(self.h, b.h))
    def add(self, b): check(lib().te_vec_add(self.h, b.h))
    def multiply(self, b): check(lib().te_vec_multiply(self.h, b.h))  # v[i] *= b[i] (any one kind of vector)

    def addScaled(self, alpha, a, beta=None, b=None):
        if b is None:
            check(lib().te_vec_add_scaled(self.h, alpha, a.h))
        else:
            check(lib().te_vec_add_scaled2(self.h, alpha, a.h, beta, b.h))

    def scaleThenAdd(self, alpha, b): check(lib().te_vec_scale_then_add(self.h, alpha, b.h))

    def scaleThenAddScaled(self, alpha, beta, b, gamma=None, c=None):
        if c is None:
            check(lib().te_vec_scale_then_add_scaled(self.h, alpha, beta, b.h))
        else:
            check(lib().te_vec_scale_then_add_scaled2(self.h, alpha, beta, b.h, gamma, c.h))

    def twoNormSqLocal(self):
        out = C.c_double()
        check(lib().te_vec_two_norm_sq(self.h, C.byref(out)))
        return out.value

    def twoNorm(self):
        return float(np.sqrt(self.twoNormSqLocal()))

    def infNorm(self):
        out = C.c_double()
        check(lib().te_vec_inf_norm(self.h, C.byref(out)))
        return out.value

    def dot(self, b):
        out = C.c_double()
        check(lib().te_vec_dot(self.h, b.h, C.byref(out)))
        return out.value

    def checksumLocal(self):
        """this rank's part of te_vec_checksum (sum modulo 2^64 of the values' bit patterns); see combine_checksums"""
        out = C.c_uint64()
        check(lib().te_vec_checksum(self.h, C.byref(out)))
        return int(out.value)

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None and getattr(self.gmg, "h", None):
            _lib.te_vec_destroy(self.h)
            self.h = None


class GMG:
    """Device-resident level stack: the product of CycleFactory3d::getCycle (CycleFactory3d.cpp:69-134).

    apply / smooth / restrict / interpolate / cycle carry the reference plugin names
    (Operator::apply, Smoother::smooth, Restrictor::restrict, Interpolator::interpolate,
    Cycle::apply)."""

    def __init__(self, hier, device=-1):
        self.hier = hier
        self.h = C.c_void_p()
        check(lib().te_gmg_create(hier.h, device, C.byref(self.h)))
        self.num_levels = lib().te_gmg_num_levels(self.h)
        self._cb = None

    @staticmethod
    def default_opts(**kw):
        o = CycleOpts()
        lib().te_cycle_opts_default(C.byref(o))
        for k, v in kw.items():
            if not hasattr(o, k):
                raise AttributeError(k)
            setattr(o, k, v)
        return o

    def new_vector(self, level=0, data=None):
        return Vec(self, level, data)

    def new_iface_vector(self, level=0, data=None):
        return Vec(self, level, data, iface=True)

    # ---- boundary data on the device (one kind per side of the domain: Hierarchy(neumann_sides=...))
    def new_boundary_vector(self, level=0, data=None):
        return Vec(self, level, data, boundary=True)

    # ---- MAC gradient, divergence, pressure projection (te_hip.h: they replace nothing in the reference)
    def new_face_vector(self, level=0, data=None):
        return Vec(self, level, data, faces=True)

    def gradient(self, u, G, bdata=None, level=0):
        """G = grad u on the cell faces, ghosts as te_apply reads them, boundary data from `bdata` (None: zero); collective"""
        check(lib().te_gradient(self.h, level, u.h, bdata.h if bdata is not None else None, G.h))

    def divergence(self, U, out, alpha=1.0, level=0):
        """out = alpha div U (patch-local)"""
        check(lib().te_divergence(self.h, level, float(alpha), U.h, out.h))

    def project(self, U, p, alpha=1.0, bdata=None, level=0):
        """U -= alpha grad p in one pass; collective"""
        check(lib().te_project(self.h, level, float(alpha), p.h, bdata.h if bdata is not None else None, U.h))

    # ---- a variable-density step on the device (te_hip.h te_faces_from_cells): coefficient from a cell field, weighted projection, fold
    def faces_from_cells(self, c, F, mode=FACE_MEAN, cb=None, level=0):
        """F = the face values of the cell field c (FACE_MEAN, FACE_HARMONIC or FACE_RECIP_MEAN); cb: the field's values on the
        physical faces, a boundary vector (None: the cell just inside). Single rank."""
        check(lib().te_faces_from_cells(self.h, level, int(mode), c.h, cb.h if cb is not None else None, F.h))

    def project_weighted(self, U, p, w, alpha=1.0, bdata=None, level=0):
        """U -= alpha (w (.) grad p) in one pass, w a face vector distinct from U; collective"""
        check(lib().te_project_weighted(self.h, level, float(alpha), p.h, bdata.h if bdata is not None else None, w.h, U.h))

    def add_boundary_rhs_weighted(self, bdata, w, f, level=0):
        """add_boundary_rhs with every datum multiplied first by the face weight w on its physical face, in place"""
        check(lib().te_add_boundary_rhs_weighted(self.h, level, bdata.h, w.h, f.h))

    # ---- transport of a cell field by a face velocity (te_hip.h te_advect_flux): donor-cell flux, update, matching, rate. Single rank.
    def advect_flux(self, U, c, F, cb=None, level=0):
        """F = U (.) c_upwind, matched on coarse/fine faces; cb: the field's values on the physical faces (None: the cell just inside)"""
        check(lib().te_advect_flux(self.h, level, U.h, c.h, cb.h if cb is not None else None, F.h))

    def advect(self, U, c, out, alpha=1.0, cb=None, level=0):
        """out = c - alpha div(U c_upwind) in one pass, out distinct from c"""
        check(lib().te_advect(self.h, level, float(alpha), U.h, c.h, cb.h if cb is not None else None, out.h))

    def faces_match(self, F, level=0):
        """the coarse side's entries of every coarse/fine face <- the mean of the covering fine copies, in place"""
        check(lib().te_faces_match(self.h, level, F.h))

    def faces_max_rate(self, U, level=0):
        """max |U_a| / h_a over the stored entries of the face vector U"""
        r = C.c_double(0.0)
        check(lib().te_faces_max_rate(self.h, level, U.h, C.byref(r)))
        return r.value

    # ---- second-order limited (MUSCL) transport (te_hip.h te_cell_slopes): slopes, flux from edge states, update. Single rank.
    def cell_slopes(self, c, sx, sy, sz=None, kind=SLOPE_MC, cb=None, level=0):
        """sx, sy, sz = the slopes of the cell field c along x, y, z (SLOPE_ZERO, SLOPE_MINMOD, SLOPE_MC or SLOPE_CENTRAL); sz is
        None in 2D"""
        check(lib().te_cell_slopes(self.h, level, int(kind), c.h, cb.h if cb is not None else None, sx.h, sy.h, sz.h if sz is not None else None))

    def advect_flux_muscl(self, U, c, F, kind=SLOPE_MC, cb=None, level=0):
        """advect_flux with the cell operands replaced by the edge states c +- 0.5 S of limited slopes"""
        check(lib().te_advect_flux_muscl(self.h, level, int(kind), U.h, c.h, cb.h if cb is not None else None, F.h))

    def advect_muscl(self, U, c, out, alpha=1.0, kind=SLOPE_MC, cb=None, level=0):
        """out = c - alpha div(F), F = advect_flux_muscl's flux, never stored; out distinct from c"""
        check(lib().te_advect_muscl(self.h, level, float(alpha), int(kind), U.h, c.h, cb.h if cb is not None else None, out.h))

    # ---- the variable-coefficient operator div(beta grad u) (te_hip.h: a second path, taken while a coefficient is set)
    def set_coefficient(self, beta):
        """beta: a level-0 face vector (copied, then restricted to every level); None clears the coefficient.
        Every call clears the reaction term: per step set beta first, then sigma (set_reaction).
        Collective on a sharded hierarchy (each rank hands over its own patches' entries): blocks of beta travel to the ranks
        that hold the parents."""
        check(lib().te_gmg_set_coefficient(self.h, beta.h if beta is not None else None))

    def has_coefficient(self):
        return bool(lib().te_gmg_has_coefficient(self.h))

    def coefficient(self, level, out):
        """out (a face vector of `level`) = the solver's beta on that level: this rank's patches (a replicated level: all of it)"""
        check(lib().te_gmg_coefficient(self.h, level, out.h))

    # ---- the reaction term: div(beta grad u) - sigma u (te_hip.h te_gmg_set_reaction; only while a coefficient is set)
    def set_reaction(self, sigma):
        """sigma: a level-0 cell vector, every entry >= 0 (copied, then restricted to every level); None clears it.
        After set_coefficient, never before: set_coefficient clears sigma. Collective on a sharded hierarchy."""
        check(lib().te_gmg_set_reaction(self.h, sigma.h if sigma is not None else None))

    def has_reaction(self):
        return bool(lib().te_gmg_has_reaction(self.h))

    def reaction(self, level, out):
        """out (a cell vector of `level`) = the solver's sigma on that level: this rank's patches"""
        check(lib().te_gmg_reaction(self.h, level, out.h))

    # ---- the coarsest level of the cycle with a coefficient (te_hip.h te_gmg_set_coef_coarse): a property of the solver
    def set_coef_coarse(self, kind, sub_n=0, cycles=2):
        """COEF_COARSE_SWEEPS (default: coarse_sweeps sweeps) or COEF_COARSE_SUBCYCLE: a one-patch coarsest level is split into
        patches of sub_n cells per axis (0: in 3D 8 where valid, else the smallest valid size) and solved by `cycles` cycles of an auxiliary solver.
        Sharded: every rank calls it; the ranks that hold the coarsest patch run the (single-rank) auxiliary solver"""
        check(lib().te_gmg_set_coef_coarse(self.h, int(kind), int(sub_n), int(cycles)))

    def coef_coarse(self):
        """-> (kind, resolved sub_n, cycles)"""
        k, s, c = C.c_int(), C.c_int(), C.c_int()
        check(lib().te_gmg_coef_coarse(self.h, C.byref(k), C.byref(s), C.byref(c)))
        return k.value, s.value, c.value

    def faces_restrict(self, fine_level, fine, coarse):
        """coarse (a face vector of fine_level + 1) = the face average of fine; collective"""
        check(lib().te_faces_restrict(self.h, fine_level, fine.h, coarse.h))

    def add_boundary_rhs(self, bdata, f, level=0):
        """f -= 2 g / h^2 on Dirichlet faces, f +- g_n / h on Neumann faces (Init.cpp:186-240, :89-146), in place"""
        check(lib().te_add_boundary_rhs(self.h, level, bdata.h, f.h))

    def boundary_sample(self, bdata, problem=0, level=0):
        """the canned problems' boundary data: exact on Dirichlet faces, the derivative along the axis on Neumann faces"""
        check(lib().te_boundary_sample(self.h, level, problem, bdata.h))

    def init_problem_sides(self, f, exact=None, problem=0, level=0):
        """init_problem with the kind of every physical face taken from the hierarchy's side mask"""
        check(lib().te_init_problem_sides(self.h, level, problem, f.h, exact.h if exact is not None else None))

    # ---- the Schur-complement route (SchurHelper.h), single rank
    def iface_interp(self, u, gamma, level=0): check(lib().te_iface_interp(self.h, level, u.h, gamma.h))
    def apply_with_interface(self, u, gamma, f, level=0): check(lib().te_apply_with_interface(self.h, level, u.h, gamma.h, f.h))
    def add_iface_rhs(self, gamma, f, level=0): check(lib().te_add_iface_rhs(self.h, level, gamma.h, f.h))

    def solve_with_interface(self, f, u, gamma, diff=None, level=0):
        check(lib().te_solve_with_interface(self.h, level, f.h, u.h, gamma.h, diff.h if diff is not None else None))

    def schur_apply(self, x, y, level=0): check(lib().te_schur_apply(self.h, level, x.h, y.h))
    def schur_cheb(self, x, y, level=0): check(lib().te_schur_cheb(self.h, level, x.h, y.h))

    def schur_solve(self, f, u, gamma, prec=SCHUR_PREC_NONE, max_it=1000, tol=1e-12, level=0):
        """-> (iterations, final relative residual); gamma: initial guess in, solution out"""
        its, rr = C.c_int(), C.c_double()
        check(lib().te_schur_solve(self.h, level, int(prec), f.h, u.h, gamma.h, max_it, tol, C.byref(its), C.byref(rr)))
        return its.value, rr.value

    def sync(self):
        check(lib().te_gmg_sync(self.h))

    def stream(self):
        return lib().te_gmg_stream(self.h)

    def apply(self, u, f, level=0): check(lib().te_apply(self.h, level, u.h, f.h))
    def residual(self, u, f, r, level=0): check(lib().te_residual(self.h, level, u.h, f.h, r.h))
    def residual_norm_sq(self, u, f, r, level=0):
        """r = f - A u and this rank's part of ||r||^2, formed by the residual kernel itself"""
        out = C.c_double()
        check(lib().te_residual_norm_sq(self.h, level, u.h, f.h, r.h, C.byref(out)))
        return out.value

    def patch_apply(self, u, f, level=0): check(lib().te_patch_apply(self.h, level, u.h, f.h))
    def verify_schedule(self, opts): check(lib().te_gmg_verify_schedule(self.h, C.byref(opts)))

    def autotune(self, opts, reps=10):
        """te_gmg_autotune (collective): -> (ms per cycle of the chosen form, report line)"""
        ms, buf = C.c_double(), C.create_string_buffer(1024)
        check(lib().te_gmg_autotune(self.h, C.byref(opts), reps, C.byref(ms), buf, 1024))
        return ms.value, buf.value.decode()

    def use_push(self, enable=True):
        """the direct-store transport (te_gmg_use_push): collective"""
        check(lib().te_gmg_use_push(self.h, int(bool(enable))))

    def push_failed(self):
        """0, or the first failure's code of the direct-store transport (1 a wait gave up, 2 a peer's flag two exchanges
        ahead, 3 a peer behind when its buffer was overwritten, 4 epochs out of sequence)"""
        return int(lib().te_gmg_push_failed(self.h))

    def set_patch_bcgs(self, tol=1e-12, max_it=1000):
        """BiCGStabSolver(op, tol, max_it), PatchSolvers/BiCGStabSolver.h:103-108"""
        check(lib().te_gmg_set_patch_bcgs(self.h, float(tol), int(max_it)))

    def patch_bcgs_iterations(self, level, n_local):
        import numpy as np
        its = np.zeros(max(int(n_local), 1), dtype=np.int32)
        check(lib().te_gmg_patch_bcgs_iterations(self.h, level, its.ctypes.data_as(_P)))
        return its[:n_local]

    def comm_info(self):
        """(ranks, rank) of the native RCCL communicator, (0, -1) without one"""
        a, b = C.c_int(), C.c_int()
        check(lib().te_gmg_comm_info(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_option(self, name, value="1"):
        """one TE_* switch of this solver (they are read from the environment once, at creation); None clears it"""
        check(lib().te_gmg_set_option(self.h, name.encode(), None if value is None else str(value).encode()))

    def slab_count(self, level, kind=0):
        """z-slabs per patch of the 3D kernels of `level` as the switches stand (SLABS_STENCIL or SLABS_SWEEP)"""
        zs = C.c_int()
        check(lib().te_gmg_slab_count(self.h, level, kind, C.byref(zs)))
        return zs.value

    def release_workspace(self):
        """hand te_bicgstab's work vectors (8 x a level-0 vector) and te_fmg's back"""
        check(lib().te_gmg_release_workspace(self.h))

    def set_allreduce(self, fn):
        """fn(list of floats, op) -> list of floats (op 0 sum, 1 max), the same on every rank"""
        def cb(user, vals, n, op):
            try:
                out = fn([vals[i] for i in range(n)], op)
                for i in range(n):
                    vals[i] = out[i]
                return 0
            except Exception:  # never let an exception cross the C boundary
                import traceback
                traceback.print_exc()
                return 1
        self._ar = ALLREDUCE_FN(cb)
        check(lib().te_gmg_set_allreduce(self.h, self._ar, None))

    def smooth(self, f, u, level=0, smoother=SMOOTH_PATCH_SOLVE, omega=6.0 / 7.0, sweeps=1):
        check(lib().te_smooth(self.h, level, f.h, u.h, smoother, omega, sweeps))

    def restrict(self, coarse, fine, fine_level=0): check(lib().te_restrict(self.h, fine_level, fine.h, coarse.h))
    def interpolate(self, coarse, fine, fine_level=0): check(lib().te_prolong_add(self.h, fine_level, coarse.h, fine.h))
    def interpolate_linear(self, coarse, fine, fine_level=0):
        """Interpolator::interpolate with the tri-/bilinear interpolator (TE_INTERP_LINEAR), whatever the solver's setting"""
        check(lib().te_prolong_linear_add(self.h, fine_level, coarse.h, fine.h))

    def interpolate_quadratic(self, coarse, fine, fine_level=0):
        """the FMG interpolation te_prolong_quadratic: fine = Pi coarse (sets; reads no boundary data)"""
        check(lib().te_prolong_quadratic(self.h, fine_level, coarse.h, fine.h))

    def boundary_restrict(self, fine_bdata, coarse_bdata, fine_level=0):
        """the boundary vector of level fine_level + 1: means of the 2^(dim-1) fine face entries that cover a coarse one"""
        check(lib().te_boundary_restrict(self.h, fine_level, fine_bdata.h, coarse_bdata.h))

    def fmg(self, f, u, opts, bdata=None, cycles=2):
        """te_fmg: full multigrid from the INTERIOR right-hand side f and the level-0 boundary vector (None: homogeneous data),
        `cycles` cycles per level with opts and the solver's interpolator -> the relative residual |F - A u| / |F|"""
        rr = C.c_double()
        check(lib().te_fmg(self.h, C.byref(opts), f.h, bdata.h if bdata is not None else None, u.h, int(cycles), C.byref(rr)))
        return rr.value

    def patch_indicator(self, u, level=0):
        """te_patch_indicator: per local patch, the largest undivided second difference of u inside the patch"""
        out = np.zeros(max(self.hier.sizes(level)[0], 1), np.float64)
        check(lib().te_patch_indicator(self.h, level, u.h, _ptr(out)))
        return out[:self.hier.sizes(level)[0]]

    def set_interpolator(self, kind):
        """which prolongation cycle() and bicgstab() use: INTERP_DIRECT (default) or INTERP_LINEAR"""
        check(lib().te_gmg_set_interpolator(self.h, int(kind)))

    @property
    def interpolator(self):
        kind = lib().te_gmg_interpolator(self.h)
        if kind < 0:
            check(kind)
        return kind

    def cycle(self, opts, f, u): check(lib().te_vcycle(self.h, C.byref(opts), f.h, u.h))

    def bicgstab(self, x, b, opts=None, max_it=1000, tol=1e-12):
        its, rr = C.c_int(), C.c_double()
        check(lib().te_bicgstab(self.h, C.byref(opts) if opts is not None else None, x.h, b.h, max_it, tol,
                                C.byref(its), C.byref(rr)))
        return its.value, rr.value

    def init_problem(self, f, exact=None, problem=0, neumann=False, level=0):
        """Init::initDirichlet / initNeumann for the canned problems (0 trig, 1 gauss, 2 random rhs), on the device"""
        check(lib().te_init_problem(self.h, level, problem, int(neumann), f.h, exact.h if exact is not None else None))

    def integrate(self, v, level=0):
        """Domain<D>::integrate (Domain.h:258-278), this rank's part"""
        out = C.c_double()
        check(lib().te_integrate(self.h, level, v.h, C.byref(out)))
        return out.value

    def volume(self, level=0):
        """Domain<D>::volume (Domain.h:237-251), this rank's part"""
        out = C.c_double()
        check(lib().te_volume(self.h, level, C.byref(out)))
        return out.value

    def setup_ms(self):
        """where te_gmg_create spent its time (include/te_hip.h te_gmg_setup_ms), by name"""
        v = (C.c_double * 8)()
        check(lib().te_gmg_setup_ms(self.h, v, 8))
        names = ("context_streams", "host_tables", "device_allocations", "device_allocation_count", "table_uploads", "work_vectors", "final_sync", "total")
        return {k: (int(x) if k.endswith("count") else round(float(x), 3)) for k, x in zip(names, v)}

    def profile(self, enable=True): check(lib().te_gmg_profile(self.h, int(enable)))
    def profile_reset(self): check(lib().te_gmg_profile_reset(self.h))
    def profile_select(self, name=None): check(lib().te_gmg_profile_select(self.h, (name or "").encode()))
    def profile_stride(self, stride=1): check(lib().te_gmg_profile_stride(self.h, int(stride)))

    def profile_rows(self):
        names = (C.c_char * 64 * 64)()
        calls = (C.c_int64 * 64)()
        ms = (C.c_double * 64)()
        cells = (C.c_int64 * 64)()
        n = lib().te_gmg_profile_rows(self.h, 64, names, calls, ms, cells)
        if n < 0:
            check(n)
        return {bytes(names[i]).split(b"\0")[0].decode(): dict(calls=calls[i], ms=ms[i], cells=cells[i])
                for i in range(n)}

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.te_gmg_destroy(self.h)
            self.h = None
