// Layout facts that the kernels and the host-side table builder (level_tables.cpp) share: the face kinds and the sizes and
// element orders of the patch-solve tables. No device header is included: this file also compiles with the plain host compiler.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define TE_HOST_DEVICE __host__ __device__
#else
#define TE_HOST_DEVICE
#endif

namespace te
{
enum FaceKind : int32_t { FACE_DIRICHLET = 0, FACE_NEUMANN = 1, FACE_LOCAL = 2, FACE_GHOST = 3 };

// patchsolve32.hpp: where element e of lane `lane` of the three-pass kernels' matrix m sits in the row-major 32 x 32 matrix
// (the operand layouts are described there, above loadMatFrag)
TE_HOST_DEVICE inline int matFragSource(int m, int lane, int e)
{
	const int j = lane & 15, g = lane >> 4;
	if (m == 0 || m == 3) return (2 * j + (e >> 3)) * 32 + 4 * (e & 7) + g;
	if (m == 2) return (16 * (e >> 3) + j) * 32 + 4 * (e & 7) + g;
	return (16 * (e >> 3) + j) * 32 + 16 * ((e >> 2) & 1) + g + 4 * (e & 3);
}

// patchsolve32_sym.hpp (k_ps_sym): the fragment-ordered half matrices of one plan, [transform 6][parity 2][k-step 4][lane 64],
// and one table of reciprocal eigenvalue sums
constexpr int PSS_FRAG = 6 * 2 * 4 * 64;
constexpr int PSS_INV  = 32 * 32 * 32;

// kernels2d.hpp (k_patch_solve2d_sym): the matrix fragments of one plan, [stage 4][k-step 8][t 4][lane 64]
constexpr int PS2S_STAGE = 8 * 4 * 64, PS2S_PLAN = 4 * PS2S_STAGE;
} // namespace te
