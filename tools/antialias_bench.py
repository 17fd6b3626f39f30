"""Edge-antialiasing timing on one idle MI355X: the new pass (gif_amd.antialias) next to the rasteriser passes it
follows, from the same run.  Workload: the FLAME-sized sphere of tests/test_gpu_render_grad.py (V = 5023, F = 9976), B = 4, 256 x 256,
C = 4 (three attribute channels and the mask, as rasterize_attributes_aa runs it).
  entry points   one C-ABI call on prepared buffers: gif_antialias_f32, gif_antialias_bwd_f32 (both gradients, and each alone)
                 next to gif_rasterize_colors_f32 and gif_rasterize_colors_bwd_f32 (both gradients)
  functions      the autograd functions users call, forward and backward apart: antialias, rasterize_attributes, and
                 rasterize_attributes_aa (rasteriser + antialias) as a whole
Each figure is the median over `--calls` eager calls (after `--warmup`) of the time between two HIP events around one call, so it
includes the gaps the host leaves between the launches of a call; at these sizes (tens of microseconds of kernel time) the
function figures are mostly host time.  No time is required of the new kernels: there is no earlier version.
--max-hops H adds, next to those rows, the walking entry points gif_antialias_walk_f32 / gif_antialias_walk_bwd_f32 (DESIGN.md
§3p) and the three functions at max_hops = H; the rows without a hop count in the same run are the yardstick for what walking
costs.  --coverage adds how much of the outline blends at 0, 4, 8 and 16 hops, counted by the float64 restatement
(tests/antialias_walk_ref.py) on the GPU's tri and depth buffers.
Usage (GPU): python tools/antialias_bench.py [--batch 4] [--size 256] [--max-hops H] [--coverage] [--out profiles/antialias.txt]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from flame_bench import median_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--max-hops", type=int, default=None, help="also time the walking entry points and functions at this setting")
    ap.add_argument("--coverage", action="store_true", help="count the outline pairs that blend at 0 / 4 / 8 / 16 hops")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "antialias_bench needs an MI355X"
    from test_gpu_render_grad import sphere_mesh
    from gif_amd import _lib, render
    from gif_amd import antialias as AA
    from gif_amd import standard_rasterize as sr
    B, h, w, C = a.batch, a.size, a.size, 4
    v, f = sphere_mesh(B)
    vt, ft = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    F = ft.shape[0]
    attr = torch.rand(v.shape, generator=torch.Generator().manual_seed(0)).cuda()
    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream

    # prepared buffers for the entry points
    faces_b = ft[None].expand(B, -1, -1)
    fv = sr.face_vertices(sr.to_image_space(vt, h, w), faces_b)
    fc = sr.face_vertices(attr, faces_b)
    depth, tri, img = sr.new_buffers(B, h, w, "cuda")
    sr.standard_rasterize_colors(fv, fc, depth, tri, img, h, w)
    adj = AA.edge_adjacency(ft)
    image = torch.cat((img.permute(0, 3, 1, 2), (tri >= 0)[:, None].float()), 1).contiguous()
    out, gi, gfv, gfc = torch.empty_like(image), torch.empty_like(image), torch.empty_like(fv), torch.empty_like(fc)
    g4, g3 = torch.randn_like(image), torch.randn_like(img)
    ws_aa = torch.empty(lib.gif_antialias_bwd_workspace_bytes(B, F, h, w) // 4, device="cuda")
    ws_rb = torch.empty(lib.gif_rasterize_colors_bwd_workspace_bytes(B, F, h, w) // 4, device="cuda")
    ptr = lambda t: t.data_ptr()

    def aa_fwd():
        _lib.check(lib.gif_antialias_f32(ptr(image), ptr(tri), ptr(depth), ptr(fv), ptr(adj), ptr(out), B, C, F, h, w, stream), "aa")

    def aa_bwd(need_i=True, need_v=True):
        _lib.check(lib.gif_antialias_bwd_f32(ptr(image), ptr(tri), ptr(depth), ptr(fv), ptr(adj), ptr(g4), ptr(gi) if need_i else None,
                                             ptr(gfv) if need_v else None, B, C, F, h, w, ptr(ws_aa), stream), "aa_bwd")

    def rast_fwd():  # (on buffers that already hold the result: the same faces win again)
        sr.standard_rasterize_colors(fv, fc, depth, tri, img, h, w)

    def rast_bwd():
        _lib.check(lib.gif_rasterize_colors_bwd_f32(ptr(fv), ptr(fc), ptr(tri), ptr(g3), ptr(gfv), ptr(gfc), B, F, h, w, ptr(ws_rb),
                                                    stream), "rast_bwd")

    # the functions
    vg, ag, ig = vt.clone().requires_grad_(True), attr.clone().requires_grad_(True), image.clone().requires_grad_(True)
    o_aa = AA.antialias(ig, tri, depth, vg, ft)
    o_ra, _ = render.rasterize_attributes(vg, ft, ag, h, w)
    G3 = torch.randn_like(o_ra)

    def whole_aa():
        i2, c2 = AA.rasterize_attributes_aa(vg, ft, ag, h, w)
        return torch.autograd.grad([i2, c2], [vg, ag], [G3, g4[:, 3:]])

    def whole_ra():
        return torch.autograd.grad(render.rasterize_attributes(vg, ft, ag, h, w)[0], [vg, ag], G3)

    hops = a.max_hops

    def walk_fwd():
        _lib.check(lib.gif_antialias_walk_f32(ptr(image), ptr(tri), ptr(depth), ptr(fv), ptr(adj), ptr(out), B, C, F, h, w, hops,
                                              stream), "aa_walk")

    def walk_bwd(need_i=True, need_v=True):
        _lib.check(lib.gif_antialias_walk_bwd_f32(ptr(image), ptr(tri), ptr(depth), ptr(fv), ptr(adj), ptr(g4),
                                                  ptr(gi) if need_i else None, ptr(gfv) if need_v else None, B, C, F, h, w, hops,
                                                  ptr(ws_aa), stream), "aa_walk_bwd")

    def whole_aa_walk():
        i2, c2 = AA.rasterize_attributes_aa(vg, ft, ag, h, w, max_hops=hops)
        return torch.autograd.grad([i2, c2], [vg, ag], [G3, g4[:, 3:]])

    def sil_walk(max_hops):
        vs = vt.clone().requires_grad_(True)
        return lambda: torch.autograd.grad(AA.soft_silhouette(vs, ft, h, w, max_hops=max_hops), vs, g4[:, 3:])

    arms = [
        ("gif_antialias_f32", aa_fwd),
        ("gif_antialias_bwd_f32 (image + vertices)", aa_bwd),
        ("gif_antialias_bwd_f32 (image only)", lambda: aa_bwd(True, False)),
        ("gif_antialias_bwd_f32 (vertices only)", lambda: aa_bwd(False, True)),
        ("gif_rasterize_colors_f32", rast_fwd),
        ("gif_rasterize_colors_bwd_f32", rast_bwd),
        ("antialias() forward", lambda: AA.antialias(ig, tri, depth, vg, ft)),
        ("antialias() backward", lambda: torch.autograd.grad(o_aa, [ig, vg], g4, retain_graph=True)),
        ("rasterize_attributes() forward", lambda: render.rasterize_attributes(vg, ft, ag, h, w)),
        ("rasterize_attributes() backward", lambda: torch.autograd.grad(o_ra, [vg, ag], G3, retain_graph=True)),
        ("rasterize_attributes() fwd + bwd", whole_ra),
        ("rasterize_attributes_aa() fwd + bwd", whole_aa),
    ]
    if hops is not None:
        o_walk = AA.antialias(ig, tri, depth, vg, ft, max_hops=hops)
        tag = f"max_hops={hops}"
        arms += [
            (f"gif_antialias_walk_f32, {tag}", walk_fwd),
            (f"gif_antialias_walk_bwd_f32 (image + vertices), {tag}", walk_bwd),
            (f"gif_antialias_walk_bwd_f32 (image only), {tag}", lambda: walk_bwd(True, False)),
            (f"gif_antialias_walk_bwd_f32 (vertices only), {tag}", lambda: walk_bwd(False, True)),
            (f"antialias({tag}) forward", lambda: AA.antialias(ig, tri, depth, vg, ft, max_hops=hops)),
            (f"antialias({tag}) backward", lambda: torch.autograd.grad(o_walk, [ig, vg], g4, retain_graph=True)),
            (f"rasterize_attributes_aa({tag}) fwd + bwd", whole_aa_walk),
            ("soft_silhouette() fwd + bwd", sil_walk(0)),
            (f"soft_silhouette({tag}) fwd + bwd", sil_walk(hops)),
        ]
    pairs = int(((tri[:, :, 1:] != tri[:, :, :-1]).sum() + (tri[:, 1:] != tri[:, :-1]).sum()).item())
    aa_fwd()
    moved = int((out != image).any(1).sum().item())
    if hops is not None:
        walk_fwd()
        moved_walk = int((out != image).any(1).sum().item())
    res = {}
    for _ in range(2):  # two alternating passes; the second is reported (clocks and caches settled)
        for name, fn in arms:
            res[name] = median_ms(fn, a.calls, a.warmup)
    lines = [f"edge antialiasing, sphere V = {v.shape[1]}, F = {F}, B = {B}, {h} x {w}, C = {C}; {torch.cuda.get_device_name(0)}",
             f"{pairs} pixel pairs with different faces, {moved} pixels changed by the blend, "
             f"coverage {(tri >= 0).float().mean().item():.3f}",
             f"median of {a.calls} eager calls after {a.warmup} warm-up calls, HIP events around each call (10th .. 90th percentile)"]
    if hops is not None:
        lines.insert(2, f"{moved_walk} pixels changed by the blend with max_hops = {hops}")
    for name, _ in arms:
        m, lo, hi = res[name]
        lines.append(f"{name:60s} {m * 1e3:9.1f} us  ({lo * 1e3:.1f} .. {hi * 1e3:.1f})")
    if a.coverage:
        import antialias_ref as aref
        import antialias_walk_ref as wref
        cov = (tri >= 0)[:, None].double().cpu()
        fv64 = aref.face_vertices_ref(vt.cpu().double(), sr.to_image_space(vt, h, w).cpu(), f, h, w)
        adj64 = aref.edge_adjacency_ref(f)
        lines.append("coverage of the outline (float64 restatement on the GPU's tri and depth, coverage as the image, all images):")
        for n in (0, 4, 8, 16):
            o, st = wref.antialias_walk_ref(cov, tri.cpu(), depth.cpu(), fv64, adj64, n)
            lines.append(f"  max_hops = {n:2d}: {st['outline_pairs']} outline pairs, {int(st['hits'][:, 7].sum())} of them blend; "
                         f"{st['blended']} of all {st['pairs']} pairs blend, {st['marginal']} marginal; "
                         f"{int((o != cov).sum())} pixels changed")
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
