"""The test oracle for per-object motion vectors of draw scenes (include/soc_rt.h "Draw scenes: per-object motion
vectors"): a float32 numpy restatement of the velocity channel of the G-buffer resolve for a draw scene
with a previous-transform array.

Per covered pixel, the winning triangle's three vertices go through the C oracle's chain (oracle/soc_oracle.c,
soc_oracle_gbuffer_resolve) operation for operation, every intermediate rounded to float32 as the C does:
  clip vertex   wp = M . p, c = vp . wp, X = (c.x 0.5 + c.w 0.5) W, Y likewise           (rs_clip_vertex)
  edges         the adjugate rows of [v0 v1 v2], v = (X, Y, w), negated when det < 0    (rs_edges)
  barycentrics  e_i = r_i . (x + 0.5, y + 0.5, 1), es = e0 + e1 + e2, b1 = e1 / es, b2 = e2 / es, b0 = 1 - b1 - b2
  velocity      cc_k = vp . (M . p_k), pc_k = prev_vp . (M_prev . p_k); both interpolated with b; then
                ((cx / cw) 0.5 + 0.5) - ((px / pw) 0.5 + 0.5), and the same in y; (vx, vy, 0, 1) as RGBA16F
M is the draw's current model matrix and M_prev the SAME draw's model matrix in the previous array: the one place this
differs from the C oracle, which uses M for both (the reference, g_buffer_generation.inl:171). With previous == current
it is the C oracle's velocity bit for bit (tests/test_motion_oracle.py). A material with SOC_MATERIAL_ZERO_VELOCITY
writes 0; an empty pixel the clear value (0, 0, 0, 1).

Scene, entities_for(phase), frame_globals and the composed visibility are tests/draws_oracle.py's.
"""
import numpy as np

import draws_oracle as D
from soc_real_time_renderer_amd import raster

F = np.float32


def mat_vec4(m, x, y, z, w):
    """The oracle's mat_vec4: column-major m[16] (float32), summed left to right; x, y, z, w float32 arrays."""
    return [m[0 + i] * x + m[4 + i] * y + m[8 + i] * z + m[12 + i] * w for i in range(4)]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def pixel_triangles(sc, vis):
    """Of a composed visibility buffer: (ys, xs) of the covered pixels, their draw index and their triangle's three
    vertex indices into the scene's vertex arrays (vertex_offset applied), shape (n, 3)."""
    tri = raster.visibility_triangles(vis)
    win = D.winner_draw(sc, vis)
    base = D.triangle_bases(sc)
    ys, xs = np.nonzero(tri >= 0)
    d = win[ys, xs]
    first = np.array([dr.first_index for dr in sc["draws"]], np.int64)[d]
    off = np.array([dr.vertex_offset for dr in sc["draws"]], np.int64)[d]
    at = first + 3 * (tri[ys, xs] - base[d])
    idx = np.stack([sc["indices"][at + k].astype(np.int64) + off for k in range(3)], 1)
    return ys, xs, d, idx


def velocity(g, sc, vis, previous=None):
    """RGBA16F velocity image (H, W, 4) of the scene dict `sc` (its "transforms": (models, normal matrices) of the
    current frame) under globals g and the composed visibility buffer `vis`; `previous`: the (models, normal matrices)
    of the previous frame (None: the current ones, the reference's behaviour)."""
    H, W = vis.shape
    out = np.zeros((H, W, 4), np.float16)
    out[..., 3] = 1.0
    ys, xs, d, idx = pixel_triangles(sc, vis)
    if len(ys) == 0:
        return out
    xf = np.array([dr.transform for dr in sc["draws"]], np.int64)[d]
    cur = np.asarray(sc["transforms"][0], F).reshape(-1, 16)[xf].T            # (16, n): m[k] per pixel
    prv = cur if previous is None else np.asarray(previous[0], F).reshape(-1, 16)[xf].T
    vp = np.array(list(g.camera_projection_view_matrix), F)
    pvp = np.array(list(g.camera_previous_projection_view_matrix), F)
    one = np.ones(len(ys), F)
    Wf, Hf, half = F(W), F(H), F(0.5)
    with np.errstate(all="ignore"):
        v, cc, pc = [], [], []
        for k in range(3):
            p = sc["positions"][idx[:, k]].astype(F)
            wp = mat_vec4(cur, p[:, 0], p[:, 1], p[:, 2], one)
            c = mat_vec4(vp, *wp)
            v.append([(c[0] * half + c[3] * half) * Wf, (c[1] * half + c[3] * half) * Hf, c[3]])
            cc.append(c)
            wq = mat_vec4(prv, p[:, 0], p[:, 1], p[:, 2], one)
            pc.append(mat_vec4(pvp, *wq))
        r = [_cross(v[1], v[2]), _cross(v[2], v[0]), _cross(v[0], v[1])]
        det = v[0][0] * r[0][0] + v[0][1] * r[0][1] + v[0][2] * r[0][2]
        neg = det < 0
        r = [[np.where(neg, -c, c) for c in ri] for ri in r]
        fx, fy = xs.astype(F) + half, ys.astype(F) + half
        e = [ri[0] * fx + ri[1] * fy + ri[2] for ri in r]
        es = e[0] + e[1] + e[2]
        b1, b2 = e[1] / es, e[2] / es
        b0 = F(1.0) - b1 - b2

        def lerp(q, i):
            return b0 * q[0][i] + b1 * q[1][i] + b2 * q[2][i]
        cx, cy, cw = lerp(cc, 0), lerp(cc, 1), lerp(cc, 3)
        px, py, pw = lerp(pc, 0), lerp(pc, 1), lerp(pc, 3)
        vx = ((cx / cw) * half + half) - ((px / pw) * half + half)
        vy = ((cy / cw) * half + half) - ((py / pw) * half + half)
        flags = np.array([sc["materials"][dr.material].flags for dr in sc["draws"]], np.int64)[d]
        zero = (flags & raster.MATERIAL_ZERO_VELOCITY) != 0
        out[ys, xs, 0] = np.where(zero, F(0), vx).astype(np.float16)
        out[ys, xs, 1] = np.where(zero, F(0), vy).astype(np.float16)
    return out


PHASE_PREVIOUS, PHASE_CURRENT = 0.0, 0.35
MOVING_TRANSFORM = 1          # entities_for(phase) moves and turns entity 1 only
_CASES = {}


def case(oracle, W, H):
    """The moving case the CPU and GPU tests share, computed once per session and handed out read-only: frame 1's
    globals, current transforms entities_for(0.35), previous transforms entities_for(0.0).
    {"g", "scene" (current transforms), "previous" ((models, normal matrices)), "visibility", "reference_velocity" (the C
    oracle's: the reference's behaviour), "velocity" (this oracle's), "draw" (winning draw per pixel, -1: empty)}."""
    if (W, H) not in _CASES:
        ref = D.reference(oracle, W, H, frame=1, phase=PHASE_CURRENT)
        prev = D.with_transforms(ref["scene"], ref["g"], PHASE_PREVIOUS)["transforms"]
        c = {"g": ref["g"], "scene": ref["scene"], "previous": prev, "visibility": ref["visibility"],
             "reference_velocity": ref["gbuffer"]["velocity"],
             "velocity": velocity(ref["g"], ref["scene"], ref["visibility"], prev),
             "draw": D.winner_draw(ref["scene"], ref["visibility"])}
        for k in ("velocity", "draw"):
            c[k].setflags(write=False)
        _CASES[(W, H)] = c
    return _CASES[(W, H)]


def moving_draws(sc):
    return [i for i, dr in enumerate(sc["draws"]) if dr.transform == MOVING_TRANSFORM]
