"""The C entry points of the mesh, shading, FLAME, resize, rasteriser and antialias sources at EMPTY sizes, without a GPU.

An empty tensor has address 0, so a binding that hands an empty batch, an empty face list or an empty table to the library passes
null pointers together with a zero dimension.  Every row below is such a call: a zero dimension, every pointer null, no stream.  It
must return 0 — "nothing to do" — and it must do so before anything touches a device (this module runs where there is none: a
path that reached a launch or a hipMemsetAsync would fail here).  "null pointer" is the message for a caller's bug, a null operand
of a call that has work to do; the last row of each family shows that it is still given there.

Only paths that return before any HIP call are listed; each guard was read for it (the comment of a row names what returns).  The
zero-size paths that fill an output with zeros or copy an image (F == 0 with B * V > 0 in mesh.hip, H * W == 0 with g_sh in
shade.hip, V == 0 or no landmarks in the two FLAME backwards with their outputs given, C == 0 in gif_texture_map_f32, F == 0 with
the images given in antialias.hip) need a device: tests/test_gpu_empty_sizes.py runs them.
The *_workspace_bytes queries answer a zero dimension with a small non-negative figure (0 or 8), never a negative one.
"""
import ctypes

import pytest

from gif_amd import _lib

N = None
PARENTS5 = (ctypes.c_int32 * 5)(-1, 0, 1, 1, 1)
PARENTS1 = (ctypes.c_int32 * 1)(-1)

# (entry, arguments without the stream, what returns)
ROWS = [
    # ---- mesh.hip: (.., B, V, F)
    ("gif_vertex_normals_f32", [N] * 5 + [0, 5, 4], "B == 0"),
    ("gif_vertex_normals_f32", [N] * 5 + [2, 0, 0], "V == 0 (and F == 0)"),
    ("gif_vertex_normals_f32", [N] * 5 + [0, 0, 0], "B == 0 and V == 0"),
    ("gif_vertex_normals_f32", [N] * 5 + [0, 0, 4], "V == 0 is no longer 'bad dims'"),
    ("gif_vertex_normals_bwd_f32", [N] * 7 + [0, 5, 4], "B == 0"),
    ("gif_vertex_normals_bwd_f32", [N] * 7 + [2, 0, 0], "V == 0"),
    ("gif_face_gather_bwd_f32", [N] * 4 + [0, 5, 4], "B == 0"),
    ("gif_face_gather_bwd_f32", [N] * 4 + [2, 0, 0], "V == 0"),
    # (.., B, C, H, W, V, T)
    ("gif_texture_map_f32", [N] * 9 + [0, 3, 8, 8, 5, 4], "B == 0"),
    ("gif_texture_map_f32", [N] * 9 + [0, 0, 8, 8, 0, 4], "B == 0 with C == 0 and V == 0"),
    ("gif_texture_map_bwd_f32", [N] * 8 + [0, 3, 8, 8, 5, 4], "B == 0"),
    ("gif_texture_map_bwd_f32", [N] * 8 + [2, 0, 8, 8, 5, 4], "C == 0: no plane receives a gradient"),
    # ---- shade.hip: (.., B, Ba, H, W, T, nrm_mul, nrm_add)
    ("gif_shade_sh_f32", [N] * 6 + [0, 0, 8, 8, 4, 1.0, 0.0], "B == 0 (Ba == B)"),
    ("gif_shade_sh_f32", [N] * 6 + [0, 1, 8, 8, 4, 1.0, 0.0], "B == 0 (Ba == 1)"),
    ("gif_shade_sh_f32", [N] * 6 + [2, 2, 0, 8, 4, 1.0, 0.0], "H == 0"),
    ("gif_shade_sh_f32", [N] * 6 + [2, 1, 8, 0, 0, 1.0, 0.0], "W == 0 and T == 0"),
    ("gif_shade_sh_bwd_f32", [N] * 10 + [0, 0, 8, 8, 4, 1.0, 0.0, N], "B == 0, no output asked for"),
    ("gif_shade_sh_bwd_f32", [N] * 10 + [2, 2, 0, 8, 4, 1.0, 0.0, N], "H == 0, no output asked for"),
    ("gif_shade_sh_bwd_f32", [N] * 10 + [2, 1, 8, 0, 0, 1.0, 0.0, N], "W == 0 and T == 0, no output asked for"),
    # ---- flame.hip: skin (.., B, V, KP, J)
    ("gif_flame_skin_f32", [N] * 7 + [0, 5, 41, 5], "B == 0"),
    ("gif_flame_skin_f32", [N] * 7 + [2, 0, 41, 5], "V == 0"),
    ("gif_flame_skin_f32", [N] * 7 + [0, 0, 0, 1], "B == V == KP == 0, J = 1"),
    ("gif_flame_skin_bwd_f32", [N] * 7 + [0, 5, 41, 5, N], "B == 0"),
    ("gif_flame_skin_bwd_f32", [N] * 7 + [2, 0, 41, 5, N], "V == 0, no output asked for (nothing to zero)"),
    # joints (J0, Jdirs, parents, shape, ld, n_shape, expr, ld, n_exp, pose, ld, neck, ld, eye, ld, A, coef, B, KP, J)
    ("gif_flame_joints_f32", [N, N, PARENTS5, N, 0, 3, N, 0, 2, N, 0, N, 0, N, 0, N, N, 0, 41, 5], "B == 0"),
    ("gif_flame_joints_f32", [N, N, PARENTS5, N, 0, 0, N, 0, 0, N, 0, N, 0, N, 0, N, N, 0, 36, 5], "B == 0, no blend shapes"),
    ("gif_flame_joints_f32", [N, N, PARENTS1, N, 0, 0, N, 0, 0, N, 0, N, 0, N, 0, N, N, 0, 0, 1], "B == 0, KP == 0, J = 1"),
    # ---- flame_landmarks.hip: forward (.., B, V, J, yaw_joint, R, Ld, Ls); backward (.., B, V, R, Ld, Ls)
    ("gif_flame_landmarks_f32", [N] * 8 + [0, 5, 5, 1, 3, 1, 4], "B == 0"),
    ("gif_flame_landmarks_f32", [N] * 8 + [2, 5, 5, 1, 3, 0, 0], "Ld + Ls == 0"),
    ("gif_flame_landmarks_f32", [N] * 8 + [2, 0, 1, 0, 0, 0, 0], "V == 0, R == 0, no landmarks, J = 1"),
    ("gif_flame_landmarks_bwd_f32", [N] * 7 + [0, 5, 3, 1, 4], "B == 0"),
    ("gif_flame_landmarks_bwd_f32", [N] * 7 + [2, 0, 3, 0, 0], "V == 0"),
    # ---- resize.hip: (x, y, planes, Hi, Wi, Ho, Wo, mode)
    ("gif_resize_f32", [N, N, 0, 8, 8, 5, 7, 0], "planes == 0, bilinear"),
    ("gif_resize_f32", [N, N, 0, 8, 8, 5, 7, 1], "planes == 0, bicubic"),
    ("gif_resize_bwd_f32", [N, N, 0, 8, 8, 5, 7, 0], "planes == 0, bilinear"),
    ("gif_resize_bwd_f32", [N, N, 0, 8, 8, 5, 7, 1], "planes == 0, bicubic"),
    # ---- rasterize.hip: (.., B, F, H, W, workspace)
    ("gif_rasterize_f32", [N] * 4 + [0, 4, 8, 8, N], "B == 0"),
    ("gif_rasterize_f32", [N] * 4 + [2, 0, 8, 8, N], "F == 0 (the caller initialised the buffers)"),
    ("gif_rasterize_colors_f32", [N] * 5 + [0, 4, 8, 8, N], "B == 0"),
    ("gif_rasterize_colors_f32", [N] * 5 + [2, 0, 8, 8, N], "F == 0"),
    ("gif_rasterize_f64", [N] * 4 + [0, 4, 8, 8, N], "B == 0"),
    ("gif_rasterize_f64", [N] * 4 + [2, 0, 8, 8, N], "F == 0"),
    ("gif_rasterize_colors_f64", [N] * 5 + [0, 4, 8, 8, N], "B == 0"),
    ("gif_rasterize_colors_f64", [N] * 5 + [2, 0, 8, 8, N], "F == 0"),
    ("gif_rasterize_colors_bwd_f32", [N] * 6 + [0, 4, 8, 8, N], "B == 0"),
    ("gif_rasterize_colors_bwd_f32", [N] * 6 + [2, 0, 8, 8, N], "F == 0"),
    # ---- antialias.hip: (.., B, C, F, H, W[, max_hops][, workspace])
    ("gif_antialias_f32", [N] * 6 + [0, 3, 4, 8, 8], "B == 0"),
    ("gif_antialias_f32", [N] * 6 + [2, 3, 0, 8, 8], "F == 0, no image given"),
    ("gif_antialias_walk_f32", [N] * 6 + [0, 3, 4, 8, 8, 2], "B == 0"),
    ("gif_antialias_walk_f32", [N] * 6 + [2, 3, 0, 8, 8, 2], "F == 0, no image given"),
    ("gif_antialias_bwd_f32", [N] * 8 + [0, 3, 4, 8, 8, N], "B == 0"),
    ("gif_antialias_bwd_f32", [N] * 8 + [2, 3, 0, 8, 8, N], "F == 0, no image gradient asked for"),
    ("gif_antialias_walk_bwd_f32", [N] * 8 + [0, 3, 4, 8, 8, 2, N], "B == 0"),
    ("gif_antialias_walk_bwd_f32", [N] * 8 + [2, 3, 0, 8, 8, 2, N], "F == 0, no image gradient asked for"),
]

# (query, arguments): a zero dimension each, and all of them
WORKSPACES = [
    ("gif_rasterize_workspace_bytes", (2, 4, 8, 8)),
    ("gif_rasterize_colors_bwd_workspace_bytes", (2, 4, 8, 8)),
    ("gif_antialias_bwd_workspace_bytes", (2, 4, 8, 8)),
    ("gif_flame_skin_bwd_workspace_bytes", (2, 5, 41, 5)),
    ("gif_shade_sh_bwd_workspace_bytes", (2, 8, 8)),
]

# a call that HAS work to do and a null operand: the message stays what it was
STILL_REFUSED = [
    ("gif_vertex_normals_f32", [N] * 5 + [2, 5, 4], b"null pointer"),
    ("gif_vertex_normals_f32", [N] * 5 + [2, 5, 0], b"null output"),  # F == 0: zeros have to go somewhere
    ("gif_vertex_normals_bwd_f32", [N] * 7 + [2, 5, 4], b"null pointer"),
    ("gif_face_gather_bwd_f32", [N] * 4 + [2, 5, 4], b"null pointer"),
    ("gif_texture_map_f32", [N] * 9 + [2, 3, 8, 8, 5, 4], b"null pointer"),
    ("gif_texture_map_bwd_f32", [N] * 8 + [2, 3, 8, 8, 5, 4], b"null pointer"),
    ("gif_resize_f32", [N, N, 6, 8, 8, 5, 7, 0], b"null pointer"),
    ("gif_resize_bwd_f32", [N, N, 6, 8, 8, 5, 7, 1], b"null pointer"),
    ("gif_shade_sh_f32", [N] * 6 + [2, 2, 8, 8, 4, 1.0, 0.0], b"null pointer"),
]

# an image or texture extent of 0 where the entry point documents "bad dims": the only refusals of an empty size
BAD_DIMS = [
    ("gif_vertex_normals_f32", [N] * 5 + [-1, 5, 4]),
    ("gif_vertex_normals_f32", [N] * 5 + [2, -5, 4]),
    ("gif_texture_map_f32", [N] * 9 + [2, 3, 0, 8, 5, 4]),
    ("gif_texture_map_f32", [N] * 9 + [2, 3, 8, 0, 5, 4]),
    ("gif_texture_map_f32", [N] * 9 + [2, 3, 8, 8, 5, 0]),
    ("gif_texture_map_bwd_f32", [N] * 8 + [2, 3, 8, 8, 5, 0]),
    ("gif_resize_f32", [N, N, 0, 0, 8, 5, 7, 0]),
    ("gif_resize_f32", [N, N, 6, 8, 8, 0, 7, 0]),
    ("gif_resize_bwd_f32", [N, N, 6, 8, 8, 5, 0, 1]),
    ("gif_rasterize_f32", [N] * 4 + [2, 4, 0, 8, N]),
    ("gif_rasterize_colors_bwd_f32", [N] * 6 + [2, 4, 8, 0, N]),
    ("gif_antialias_f32", [N] * 6 + [2, 3, 4, 0, 8]),
]


def _ids(rows):
    return [f"{r[0][4:]}-{i}" for i, r in enumerate(rows)]


@pytest.mark.parametrize("entry,args,why", ROWS, ids=_ids(ROWS))
def test_zero_dimension_with_null_pointers_returns_0(entry, args, why):
    lib = _lib.load()
    rc = getattr(lib, entry)(*args, None)
    assert rc == 0, f"{entry}{tuple(args[-8:])} ({why}): rc {rc}, {lib.gif_last_error().decode(errors='replace')}"


def test_every_entry_point_of_the_seven_sources_has_a_row():
    """(a new entry point of these families needs its empty-size rows here)"""
    families = ("gif_vertex_normals", "gif_face_gather", "gif_texture_map", "gif_shade_sh", "gif_flame_", "gif_resize", "gif_rasterize",
                "gif_antialias")
    launches = {n for n in _lib.PROTOTYPES if n.startswith(families) and not n.endswith("_workspace_bytes")}
    launches.discard("gif_rasterize_assume_clean_workspace")  # takes no dimension
    assert launches == {r[0] for r in ROWS}
    queries = {n for n in _lib.PROTOTYPES if n.startswith(families) and n.endswith("_workspace_bytes")}
    assert queries == {q for q, _ in WORKSPACES}


@pytest.mark.parametrize("query,dims", WORKSPACES, ids=[q[4:] for q, _ in WORKSPACES])
def test_workspace_queries_at_a_zero_dimension(query, dims):
    fn = getattr(_lib.load(), query)
    full = fn(*dims)
    assert full > 0
    for i in range(len(dims)):
        d = list(dims)
        d[i] = 0
        n = fn(*d)
        assert n in (0, 8), (query, d, n)  # (KP == 0 with J = 5 is not a size of the skinning, KP >= 9 (J - 1): 0 as well)
    assert fn(*([0] * len(dims))) in (0, 8)


@pytest.mark.parametrize("entry,args,text", STILL_REFUSED, ids=_ids(STILL_REFUSED))
def test_a_null_operand_of_a_call_with_work_is_still_refused(entry, args, text):
    lib = _lib.load()
    assert getattr(lib, entry)(*args, None) == -1
    assert text in lib.gif_last_error(), lib.gif_last_error()


@pytest.mark.parametrize("entry,args", BAD_DIMS, ids=_ids(BAD_DIMS))
def test_negative_sizes_and_empty_images_are_bad_dims(entry, args):
    lib = _lib.load()
    assert getattr(lib, entry)(*args, None) == -1
    assert b"bad dims" in lib.gif_last_error(), lib.gif_last_error()
