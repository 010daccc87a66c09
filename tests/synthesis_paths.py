"""Which compiled code a call of the synthesis head runs: a restatement in Python of the host's choices
(tu_synthesis.hip, tu_synthesis_grad.hip: the instantiation, the chunk, the tiles) and of the kernels' own predicates
(k_synthesis.h, k_synthesis_grad.h), evaluated for every workgroup and step of a case.  tests/test_synthesis_paths_cpu.py
holds the model to the headers (tests/synthesis_paths_harness.cpp prints what the real host code chooses) and proves that
CASES reaches every instantiation with every path its family has; tests/test_synthesis_paths_gpu.py runs CASES on the
device against the twins.

A case is (n, C, dtype, D, h, w, S) with dtype "f32" or "u8" (the left frame's)."""
from collections import namedtuple

Case = namedtuple("Case", "n C dtype D h w S")

# ---- k_synthesis_grad.h ----------------------------------------------------------------------------------------------
SYG_LDS_FLOATS = 14 * 1024
SYN_LDS_FLOATS = 14 * 1024
SYN_TW, SYN_ROWS, SYN_THREADS = 64, 4, 256
SYN_TH = SYN_THREADS // SYN_TW * SYN_ROWS
MAX_PLANES = 256                                         # the entries refuse D > 256 (smx_maps.hip)

# family -> (NT, U, SC) of launch_synthesis_grad
FAMILIES = {"sc4": (10, 4, 4), "nt10": (10, 4, 0), "nt20": (20, 2, 0), "nt40": (40, 1, 0)}
FAMILY_SCALES = {"sc4": [4], "nt10": [1, 2, 3], "nt20": [5, 6, 7, 8], "nt40": list(range(9, 17))}

BACKWARD_FLAGS = ("strip_full", "strip_partial_in_full_tile", "first_j_tile", "last_j_tile_both", "ragged_j_tile",
                  "ragged_i_tile", "many_i_tiles_vboth", "later_chunk_with_terms", "chunk_without_columns",
                  "short_last_step", "vertical_one_round", "vertical_lds_table")
FORWARD_FLAGS = ("march_pairs", "march_rows", "two_chunks", "patch_groups", "patch_larger", "lanes_right_of_image",
                 "rows_below_image", "exit_past_width")


def family_of(S):
    return "sc4" if S == 4 else "nt10" if S <= 3 else "nt20" if S <= 8 else "nt40"


def family_flags(family):
    """What a family's instantiations can reach: one_round is fixed by S (U TI <= rows from S = 4 on), the LDS tap table
    exists only below; with U = 1 no step is short."""
    out = set(BACKWARD_FLAGS) - {"vertical_lds_table" if family != "nt10" else "vertical_one_round"}
    if FAMILIES[family][1] == 1:
        out.discard("short_last_step")
    return out


def reachable_flags(family, C):
    """family_flags less what the entries' D <= MAX_PLANES keeps from an instantiation: a second staged chunk needs a
    chunk shorter than D, and a gray frame's chunk is 328..352 planes in the three families with 32-row tiles."""
    out = family_flags(family)
    if all(synthesis_grad_chunk(C, MAX_PLANES, S) >= MAX_PLANES for S in FAMILY_SCALES[family]):
        out -= {"later_chunk_with_terms", "chunk_without_columns"}
    return out


def syn_grad_shape(S):
    """(rows_log2, tj_log2, NT, U)"""
    return (5, 3, 10, 4) if S <= 4 else (5, 3, 20, 2) if S <= 8 else (6, 1, 40, 1)


def syg_first(k, S):
    return 0 if k <= 0 else S * k + S // 2


def syg_t_plane(rows, tj):
    return rows * (tj + 1) + 1


def syg_row_floats(S, tj, NT, dc):
    return (S * (tj - 1) + S // 2 + NT + dc - 1) | 1


def syg_lds_floats(C, S, rows, tj, NT, U, dc):
    return C * rows * syg_row_floats(S, tj, NT, dc) + 2 * U * syg_t_plane(rows, tj) + 3 * rows


def synthesis_grad_chunk(C, D, S):
    rl, tl, NT, U = syn_grad_shape(S)
    rows, tj = 1 << rl, 1 << tl
    fixed = 2 * U * syg_t_plane(rows, tj) + 3 * rows
    dc = (SYG_LDS_FLOATS - fixed) // (C * rows) - (S * (tj - 1) + S // 2 + NT)
    dc -= dc % U
    whole = (D + U - 1) // U * U
    return U if dc < U else min(dc, whole)


def backward(case):
    """What launch_synthesis_grad chooses for a case and the set of BACKWARD_FLAGS its workgroups reach."""
    n, C, dtype, D, h, w, S = case
    rl, tl, NT, U = syn_grad_shape(S)
    ROWS, TJ = 1 << rl, 1 << tl
    TI = ROWS // S - 1
    H, W = h * S, w * S
    dc = synthesis_grad_chunk(C, D, S)
    tiles_j, tiles_i = (w + TJ - 1) // TJ, (h + TI - 1) // TI
    flags = set()
    flags.add("vertical_one_round" if U * TI <= ROWS else "vertical_lds_table")
    if tiles_i > 1:
        flags.add("many_i_tiles_vboth")                  # the last tile's row h - 1 has vboth, the others do not
    if h % TI:
        flags.add("ragged_i_tile")
    if D % U:
        flags.add("short_last_step")                     # dc is a multiple of U
    for tile in range(tiles_j):
        j_lo = tile * TJ
        j_n = min(TJ, w - j_lo)
        Ybase, Yend = syg_first(j_lo - 1, S), min(syg_first(j_lo + j_n, S), W)
        tile_full = j_lo >= 2 and j_lo + TJ <= w - 1
        if j_lo == 0:
            flags.add("first_j_tile")
        if j_lo + j_n == w:
            flags.add("last_j_tile_both")
        if j_n < TJ:
            flags.add("ragged_j_tile")
        full_steps = 0
        for d0 in range(0, D, dc):
            nd = min(dc, D - d0)
            if d0 > 0:
                flags.add("later_chunk_with_terms" if d0 < W - Ybase else "chunk_without_columns")
            for ds in range(0, nd, U):
                if tile_full and Yend + d0 + ds + U - 1 <= W:
                    full_steps += 1
                elif tile_full and full_steps:
                    flags.add("strip_partial_in_full_tile")
        if full_steps:
            flags.add("strip_full")
    fam = family_of(S)
    return {"family": fam, "instantiation": (C, dtype, fam), "rows_log2": rl, "tj_log2": tl, "NT": NT, "U": U, "dc": dc,
            "rs": syg_row_floats(S, TJ, NT, dc),
            "lds": syg_lds_floats(C, S, ROWS, TJ, NT, U, dc), "ti": TI, "tiles_i": tiles_i, "tiles_j": tiles_j,
            "threads": ROWS * TJ, "flags": flags}


# ---- k_synthesis.h -----------------------------------------------------------------------------------------------------
def syn_patch_extent(tile, S, length):
    return min((tile - 1) // S + 3, length)


def syn_left_stride(C):
    return C * SYN_TH + 1


def syn_lds_floats(C, dc, S, h, w):
    return (SYN_TW + dc - 1) * syn_left_stride(C) + syn_patch_extent(SYN_TH, S, h) * syn_patch_extent(SYN_TW, S, w) * (dc | 1)


def synthesis_chunk(C, D, S, h, w):
    elements = syn_patch_extent(SYN_TH, S, h) * syn_patch_extent(SYN_TW, S, w)
    dc = (SYN_LDS_FLOATS - (SYN_TW - 1) * syn_left_stride(C) - elements) // (syn_left_stride(C) + elements)
    return 1 if dc < 1 else min(dc, D)


def syn_i0(t, S):
    return max(2 * t + 1 - S, 0) // (2 * S)


def forward(case):
    """{"instantiations", "dc", "lds", "tiles_x", "tiles_y", "flags"} of a case; the rescaled view and the training form
    are one template with RESCALE true and false, and the device test calls both."""
    n, C, dtype, D, h, w, S = case
    H, W = h * S, w * S
    dc = synthesis_chunk(C, D, S, h, w)
    tiles_x, tiles_y = (W + SYN_TW - 1) // SYN_TW, (H + SYN_TH - 1) // SYN_TH
    flags = set()
    for ty in range(tiles_y):
        x0 = ty * SYN_TH
        if x0 + SYN_TH > H:
            flags.add("rows_below_image")
        pr_lo = syn_i0(x0, S)
        pr_n = min(syn_i0(min(x0 + SYN_TH, H) - 1, S) + 1, h - 1) - pr_lo + 1
        for wv in range(SYN_THREADS // SYN_TW):
            i0 = [syn_i0(min(x0 + wv * SYN_ROWS + j, H - 1), S) for j in range(SYN_ROWS)]
            i1 = [min(i + 1, h - 1) for i in i0]
            pairs = i0[0] == i0[1] and i1[0] == i1[1] and i0[2] == i0[3] and i1[2] == i1[3]
            flags.add("march_pairs" if pairs else "march_rows")
        for tx in range(tiles_x):
            y0 = tx * SYN_TW
            if y0 + SYN_TW > W:
                flags.add("lanes_right_of_image")
            pc_lo = syn_i0(y0, S)
            pc_n = min(syn_i0(min(y0 + SYN_TW, W) - 1, S) + 1, w - 1) - pc_lo + 1
            RC = pr_n * pc_n
            if RC < SYN_THREADS and SYN_THREADS // RC > 1:
                flags.add("patch_groups")
            if RC > SYN_THREADS:
                flags.add("patch_larger")
            chunks, d0 = 0, 0
            while d0 < D and y0 + d0 < W:
                chunks, d0 = chunks + 1, d0 + dc
            if chunks >= 2:
                flags.add("two_chunks")
            if d0 < D:
                flags.add("exit_past_width")
    return {"instantiations": [(C, dtype, True), (C, dtype, False)], "dc": dc, "lds": syn_lds_floats(C, dc, S, h, w),
            "tiles_x": tiles_x, "tiles_y": tiles_y, "flags": flags}


# ---- the case table ------------------------------------------------------------------------------------------------------
# The smallest shapes found (a greedy cover over D, h, w per instantiation and scale) at which every backward
# instantiation reaches every path it can (reachable_flags), every forward instantiation both march forms and a second
# chunk, and every scale 1..16 appears.  n = 2: the frame loop and the per-frame reload of g run twice.
CASES = [Case(*c) for c in [
    # S = 4, the compile-time scale
    (2, 3, "f32", 5, 8, 18, 4), (2, 3, "f32", 85, 1, 22, 4),
    (2, 3, "u8", 5, 8, 18, 4), (2, 3, "u8", 85, 1, 22, 4),
    (2, 1, "f32", 5, 8, 18, 4), (2, 1, "f32", 256, 1, 9, 4),
    (2, 1, "u8", 5, 8, 18, 4), (2, 1, "u8", 256, 1, 9, 4),
    # S = 1..3: the row taps from the LDS table
    (2, 3, "f32", 105, 33, 25, 1), (2, 3, "f32", 97, 1, 49, 2),
    (2, 3, "u8", 105, 33, 25, 1), (2, 3, "u8", 93, 1, 32, 3),
    (2, 1, "f32", 5, 17, 18, 2), (2, 1, "f32", 66, 9, 23, 3),
    (2, 1, "u8", 27, 33, 27, 1), (2, 1, "u8", 7, 3, 19, 3),
    # S = 5..8
    (2, 3, "f32", 5, 6, 17, 5), (2, 3, "f32", 113, 1, 8, 8),
    (2, 3, "u8", 5, 5, 17, 6), (2, 3, "u8", 65, 1, 10, 7),
    (2, 1, "f32", 5, 4, 17, 7), (2, 1, "f32", 256, 2, 18, 8),
    (2, 1, "u8", 5, 6, 17, 5), (2, 1, "u8", 7, 2, 18, 6),
    # S = 9..16: 64 x 2 tiles, 40 terms a lane
    (2, 3, "f32", 19, 7, 5, 9), (2, 3, "f32", 9, 2, 6, 16),
    (2, 3, "u8", 17, 6, 5, 10), (2, 3, "u8", 9, 2, 6, 15),
    (2, 1, "f32", 8, 5, 5, 11), (2, 1, "f32", 154, 1, 1, 14), (2, 1, "f32", 154, 1, 11, 14),
    (2, 1, "u8", 8, 5, 5, 12), (2, 1, "u8", 156, 1, 1, 13), (2, 1, "u8", 156, 1, 12, 13),
]]


def case_id(c):
    return "n%d_C%d_%s_D%d_%dx%d_S%d" % tuple(c)
