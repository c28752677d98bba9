"""Call table of the host side of the pipeline kernels (tests/test_pipeline_host_cpu.py, tools/gen_golden_pipeline_host.py):
the five workspace size queries and the 23 launch entry points of seg_eval, sr_volume, stage1_volume, sr_metrics,
seg_surface, seg_components, intensity_norm and sr_losses.

A launch row is (entry point, label, overrides of the entry point's valid call).  Pointers are dummy addresses that
nothing on the host dereferences, except the arrays the host reads itself (strides, ranks, lerp weights): those are
real ctypes arrays.  A row is called only where there is no device: an accepted call then returns REHR_EHIP instead of
launching on the dummy pointers.  What every row returned when tests/golden/pipeline_host.json was recorded is in that
file; the comments here say why a row is there.  "+k" = a pointer k bytes past an aligned address: half of a required
alignment is the smallest offset that a check of the next weaker alignment would let through."""
import ctypes as C

NAN, INF = float("nan"), float("inf")
G = 1 << 30


def P(k):
    """Dummy device address number k, 1 MiB aligned."""
    return k << 20


def i64(*v):
    return (C.c_int64 * len(v))(*v)


def f64(*v):
    return (C.c_double * len(v))(*v)


def align16(n):
    return (n + 15) & ~15


# the documented workspace layouts (include/rehrseg_hip.h), restated so that the launch rows do not lean on the queries
def surface_bytes(n):
    return 256 * 2 * 8 + 2 * align16(8 * n) + align16(n)


def cc_bytes(n):
    return 64 + 4 * align16(4 * n)


def order_bytes(b, r):
    return align16(16 * b * r) + align16(4 * b) + b * r * 256 * 4


def tile_bytes(blocks, slots):
    return blocks * slots * 8


S4 = i64(1000, 300, 20, 1)            # element strides of a (N, D, H, W) view
S5 = i64(5000, 1000, 300, 20, 1)      # ... of a (N, C, D, H, W) view

# entry point -> (argument names in call order, the valid call)
CALLS = {
    # ------------------------------------------------------------------------------------------------ seg_eval.hip
    "rehr_tta_gather_f32": (
        "vol out D H W pad_d pad_h pad_w start_d start_h start_w d h w stream",
        dict(vol=P(1), out=P(2), D=4, H=8, W=8, pad_d=1, pad_h=2, pad_w=2, start_d=0, start_h=0, start_w=0, d=4, h=8,
             w=8)),
    "rehr_tta_blend_f16acc": (
        "pred strides C d h w gaussian logits counts Do Ho Wo od oh ow stream",
        dict(pred=P(1), strides=S5, C=2, d=4, h=8, w=8, gaussian=P(2), logits=P(3), counts=P(4), Do=6, Ho=10, Wo=10,
             od=1, oh=1, ow=1)),
    "rehr_seg_eval_finalize_f16": (
        "logits counts D H W crop_d crop_h crop_w CD CH CW labels gt stats stream",
        dict(logits=P(1), counts=P(2), D=4, H=8, W=8, crop_d=0, crop_h=1, crop_w=1, CD=4, CH=6, CW=6, labels=P(3),
             gt=P(4), stats=P(5))),
    # ------------------------------------------------------------------------------------------------ seg_surface.hip
    "rehr_seg_surface_dist_f32": (
        "pred gt D H W sd sh sw dist counts workspace workspace_bytes stream",
        dict(pred=P(1), gt=P(2), D=3, H=5, W=7, sd=1.0, sh=0.5, sw=2.0, dist=P(3), counts=P(4), workspace=P(5),
             workspace_bytes=surface_bytes(105))),
    "rehr_seg_surface_reduce_f64": (
        "dist sorted counts N out workspace workspace_bytes stream",
        dict(dist=P(1), sorted=P(2), counts=P(3), N=105, out=P(4), workspace=P(5), workspace_bytes=4096)),
    # ------------------------------------------------------------------------------------------------ seg_components.hip
    "rehr_seg_cc_roots_i32": (
        "mask D H W connectivity roots workspace workspace_bytes stream",
        dict(mask=P(1), D=3, H=5, W=7, connectivity=26, roots=P(2), workspace=P(3), workspace_bytes=cc_bytes(105))),
    "rehr_seg_cc_lesion_i64": (
        "roots_pred roots_gt N out workspace workspace_bytes stream",
        dict(roots_pred=P(1), roots_gt=P(2), N=105, out=P(3), workspace=P(4), workspace_bytes=cc_bytes(105))),
    "rehr_seg_cc_compact_i32": (
        "roots N rank labels count stream",
        dict(roots=P(1), N=105, rank=P(2), labels=P(3), count=P(4))),
    # ------------------------------------------------------------------------------------------------ intensity_norm.hip
    "rehr_order_stats_f32": (
        "x B S item_stride ranks R out workspace workspace_bytes stream",
        dict(x=P(1), B=3, S=105, item_stride=105, ranks=i64(0, 52, 104), R=3, out=P(2), workspace=P(3),
             workspace_bytes=order_bytes(3, 3))),
    "rehr_percentile_f64": (
        "stats B Q t strictly_positive out stream",
        dict(stats=P(1), B=3, Q=2, t=f64(0.25, 0.5), strictly_positive=0, out=P(2))),
    "rehr_intensity_apply_f32": (
        "x y B S x_stride y_stride mode bounds bounds_stride stream",
        dict(x=P(1), y=P(2), B=3, S=105, x_stride=105, y_stride=105, mode=0, bounds=P(3), bounds_stride=2)),
    # ------------------------------------------------------------------------------------------------ sr_volume.hip
    "rehr_minmax_f32": ("x n minmax stream", dict(x=P(1), n=105, minmax=P(2))),
    "rehr_sr_window_gather_f32": (
        "vol out X Y Z C w0 b Xp Yp stream",
        dict(vol=P(1), out=P(2), X=12, Y=13, Z=6, C=1, w0=0, b=2, Xp=16, Yp=16)),
    "rehr_sr_volume_scatter_f32": (
        "net strides b C n_out X Y w0 n_windows in_minmax img seg out_minmax stream",
        dict(net=P(1), strides=S5, b=2, C=2, n_out=4, X=12, Y=13, w0=0, n_windows=5, in_minmax=P(2), img=P(3), seg=P(4),
             out_minmax=P(5))),
    "rehr_stage2_prep_f32": (
        "img minmax taps L out X P stream",
        dict(img=P(1), minmax=P(2), taps=P(3), L=5, out=P(4), X=12, P=156)),
    "rehr_stage2_unc_u8_f32": ("u minmax out n stream", dict(u=P(1), minmax=P(2), out=P(3), n=105)),
    # ------------------------------------------------------------------------------------------------ stage1_volume.hip
    "rehr_zoom_depth_f32": (
        "vol lines n C idx w nn Z img label stream",
        dict(vol=P(1), lines=156, n=6, C=2, idx=P(2), w=P(3), nn=P(4), Z=16, img=P(5), label=P(6))),
    "rehr_bspline_prefilter_axis_f64acc_f32": (
        "x y outer n inner stream", dict(x=P(1), y=P(2), outer=12, n=6, inner=13)),
    "rehr_blur_to_slices_f32": (
        "img taps L out X Y Z axis stream", dict(img=P(1), taps=P(2), L=5, out=P(3), X=12, Y=13, Z=6, axis=0)),
    # ------------------------------------------------------------------------------------------------ sr_metrics.hip
    "rehr_sr_metrics_f32": (
        "pred ps tgt ts slog ls stgt gs N D H W data_range stats workspace workspace_bytes stream",
        dict(pred=P(1), ps=S4, tgt=P(2), ts=S4, slog=P(3), ls=S4, stgt=P(4), gs=S4, N=2, D=3, H=12, W=13,
             data_range=1.0, stats=P(5), workspace=P(6), workspace_bytes=tile_bytes(6, 6))),
    # ------------------------------------------------------------------------------------------------ sr_losses.hip
    "rehr_structure_loss_fwd_f32": (
        "input istr target tstr N C D H W l1 l2 ssim sobel data_range stats loss fields workspace workspace_bytes stream",
        dict(input=P(1), istr=S5, target=P(2), tstr=S5, N=2, C=2, D=3, H=12, W=13, l1=1.0, l2=0.5, ssim=0.25, sobel=2.0,
             data_range=1.0, stats=P(3), loss=P(4), fields=P(5), workspace=P(6), workspace_bytes=tile_bytes(12, 4))),
    "rehr_structure_loss_bwd_f32": (
        "input istr target tstr N C D H W l1 l2 ssim sobel fields grad_output dinput dstr stream",
        dict(input=P(1), istr=S5, target=P(2), tstr=S5, N=2, C=2, D=3, H=12, W=13, l1=1.0, l2=0.5, ssim=0.25, sobel=2.0,
             fields=P(3), grad_output=P(4), dinput=P(5), dstr=S5)),
}
CALLS["rehr_sr_metrics_bf16"] = CALLS["rehr_sr_metrics_f32"]

# entry points whose documentation names an extent they do not take (REHR_ENOSUP)
HAS_EXTENT_LIMIT = (
    "rehr_seg_surface_dist_f32", "rehr_seg_surface_reduce_f64", "rehr_seg_cc_roots_i32", "rehr_seg_cc_lesion_i64",
    "rehr_seg_cc_compact_i32", "rehr_order_stats_f32", "rehr_percentile_f64", "rehr_intensity_apply_f32",
    "rehr_stage2_prep_f32", "rehr_zoom_depth_f32", "rehr_bspline_prefilter_axis_f64acc_f32", "rehr_blur_to_slices_f32",
    "rehr_sr_metrics_f32", "rehr_sr_metrics_bf16", "rehr_structure_loss_fwd_f32", "rehr_structure_loss_bwd_f32")


def call_args(entry, over):
    """The argument list of `entry`: its valid call with `over` on top; stream = null."""
    names, valid = CALLS[entry]
    unknown = set(over) - set(names.split())
    assert not unknown, (entry, unknown)
    vals = dict(valid, stream=None, **over)
    return [vals[n] for n in names.split()]


def _nulls(entry, *names):
    return [(entry, f"null {n}", {n: None}) for n in names]


def _off(entry, *pairs):
    """(argument, offset) -> the row with that pointer `offset` bytes past its aligned address."""
    return [(entry, f"{n} +{k}", {n: CALLS[entry][1][n] + k}) for n, k in pairs]


E = "rehr_tta_gather_f32"
ROWS = [(E, "valid", {}), (E, "valid, w % 4 != 0", dict(w=7))] + _nulls(E, "vol", "out") + [
    (E, "D = 0", dict(D=0)), (E, "w = 0", dict(w=0)), (E, "pad_d = -1", dict(pad_d=-1)),
    (E, "start_w = -1", dict(start_w=-1)),
    (E, "8 d h w = 2^40", dict(d=8192, h=4096, w=4096)),              # the limit itself is refused
    (E, "8 d h w just below 2^40", dict(d=8191, h=4096, w=4096)),
    (E, "null vol and D = 0", dict(vol=None, D=0)),
    (E, "pad_h = -1 and 8 d h w = 2^40", dict(pad_h=-1, d=8192, h=4096, w=4096)),
]

E = "rehr_tta_blend_f16acc"
ROWS += [(E, "valid", {}), (E, "valid, no gaussian pointer check", dict(gaussian=None))]
ROWS += _nulls(E, "pred", "strides", "logits", "counts") + [
    (E, "C = 0", dict(C=0)), (E, "C = 64", dict(C=64)), (E, "C = 65", dict(C=65)), (E, "d = 0", dict(d=0)),
    (E, "Wo = 0", dict(Wo=0)), (E, "od = -1", dict(od=-1)),
    (E, "od + d = Do", dict(od=2)), (E, "od + d = Do + 1", dict(od=3)), (E, "ow + w = Wo + 1", dict(ow=3)),
    (E, "negative stride", dict(strides=i64(5000, 1000, -300, 20, 1))),
    (E, "null strides and C = 65", dict(strides=None, C=65)),
    (E, "od = -1 and negative stride", dict(od=-1, strides=i64(-1, 1000, 300, 20, 1))),
]

E = "rehr_seg_eval_finalize_f16"
ROWS += [(E, "valid", {}), (E, "valid, no labels and no gt", dict(labels=None, gt=None)),
         (E, "valid, labels without gt", dict(gt=None)), (E, "valid, N % 8 != 0", dict(W=7, CW=6))]
ROWS += _nulls(E, "logits", "counts", "stats") + [
    (E, "gt without labels", dict(labels=None)),
    (E, "D = 0", dict(D=0)), (E, "CD = 0", dict(CD=0)), (E, "crop_d = -1", dict(crop_d=-1)),
    (E, "crop_h + CH = H", dict(crop_h=2)), (E, "crop_h + CH = H + 1", dict(crop_h=3)),
] + _off(E, ("logits", 1), ("counts", 1), ("logits", 2), ("logits", 8)) + [     # 2 bytes; 16 only chooses the kernel
    (E, "logits +1 and D = 0", dict(logits=P(1) + 1, D=0)),
    (E, "null stats and crop over", dict(stats=None, crop_w=3)),
]

E = "rehr_seg_surface_dist_f32"
HUGE = 1 << 40
ROWS += [(E, "valid", {}), (E, "valid 2x16x16", dict(D=2, H=16, W=16, workspace_bytes=surface_bytes(512)))]
ROWS += _nulls(E, "pred", "gt", "dist", "counts", "workspace") + [
    (E, "D = 0", dict(D=0)), (E, "W = -1", dict(W=-1)),
    (E, "H = 2048", dict(D=1, H=2048, W=1, workspace_bytes=surface_bytes(2048))),
    (E, "H = 2049", dict(D=1, H=2049, W=1, workspace_bytes=HUGE)),
    (E, "2^30 voxels", dict(D=2048, H=2048, W=256, workspace_bytes=surface_bytes(G))),
    (E, "2^30 + 2^22 voxels", dict(D=2048, H=2048, W=257, workspace_bytes=HUGE)),
    (E, "spacing 0", dict(sh=0.0)), (E, "spacing < 0", dict(sd=-1.0)), (E, "spacing NaN", dict(sw=NAN)),
    (E, "spacing inf", dict(sd=INF)),
    (E, "workspace one byte short", dict(workspace_bytes=surface_bytes(105) - 1)),
    (E, "2^30 voxels, workspace one byte short", dict(D=2048, H=2048, W=256, workspace_bytes=surface_bytes(G) - 1)),
] + _off(E, ("workspace", 8), ("dist", 2), ("counts", 4)) + [
    (E, "null pred and D = 0", dict(pred=None, D=0)),
    (E, "H = 2049 and spacing 0", dict(H=2049, sh=0.0, workspace_bytes=HUGE)),           # extent before spacing
    (E, "H = 2049 and workspace short", dict(H=2049, workspace_bytes=16)),
    (E, "spacing NaN and workspace short", dict(sd=NAN, workspace_bytes=16)),
    (E, "workspace short and workspace +8", dict(workspace=P(5) + 8, workspace_bytes=16)),
]

E = "rehr_seg_surface_reduce_f64"
ROWS += [(E, "valid", {}), (E, "valid, roomy workspace", dict(workspace_bytes=surface_bytes(105)))]
ROWS += _nulls(E, "dist", "sorted", "counts", "out", "workspace") + [
    (E, "N = 0", dict(N=0)), (E, "N = 2^30", dict(N=G)), (E, "N = 2^30 + 1", dict(N=G + 1)),
    (E, "workspace one byte short", dict(workspace_bytes=4095)),
] + _off(E, ("workspace", 4), ("workspace", 8), ("out", 4), ("counts", 4), ("dist", 2), ("sorted", 2)) + [
    (E, "N = 0 and workspace short", dict(N=0, workspace_bytes=0)),
    (E, "N = 2^30 + 1 and workspace short", dict(N=G + 1, workspace_bytes=0)),             # extent before the workspace
    (E, "null dist and N = 2^30 + 1", dict(dist=None, N=G + 1)),
    (E, "workspace short and out +4", dict(workspace_bytes=4095, out=P(4) + 4)),
]

E = "rehr_seg_cc_roots_i32"
ROWS += [(E, "valid", {}), (E, "valid, 6", dict(connectivity=6)), (E, "valid, 18", dict(connectivity=18)),
         (E, "valid 2x16x16", dict(D=2, H=16, W=16, workspace_bytes=cc_bytes(512)))]
ROWS += _nulls(E, "mask", "roots", "workspace") + [
    (E, "connectivity 8", dict(connectivity=8)),
    (E, "D = 0", dict(D=0)), (E, "W = -1", dict(W=-1)),
    (E, "2^30 voxels", dict(D=1024, H=1024, W=1024, workspace_bytes=cc_bytes(G))),
    (E, "2^30 + 2^20 voxels", dict(D=1024, H=1024, W=1025, workspace_bytes=HUGE)),
    (E, "D * H = 2^31", dict(D=65536, H=32768, W=1, workspace_bytes=HUGE)),
    (E, "workspace one byte short", dict(workspace_bytes=cc_bytes(105) - 1)),
    (E, "2^30 voxels, workspace one byte short", dict(D=1024, H=1024, W=1024, workspace_bytes=cc_bytes(G) - 1)),
] + _off(E, ("roots", 2), ("workspace", 8)) + [                    # the roots pass does not touch the workspace
    (E, "connectivity 8 and D = 0", dict(connectivity=8, D=0)),                            # EINVAL before ENOSUP
    (E, "null mask and connectivity 8", dict(mask=None, connectivity=8)),
    (E, "D = 0 and workspace short", dict(D=0, workspace_bytes=0)),
    (E, "workspace short and roots +2", dict(workspace_bytes=0, roots=P(2) + 2)),
]

E = "rehr_seg_cc_lesion_i64"
ROWS += [(E, "valid", {}), (E, "valid N = 512", dict(N=512, workspace_bytes=cc_bytes(512))),
         (E, "valid N = 1", dict(N=1, workspace_bytes=cc_bytes(1)))]
ROWS += _nulls(E, "roots_pred", "roots_gt", "out", "workspace") + [
    (E, "N = 0", dict(N=0)), (E, "N = 2^30", dict(N=G, workspace_bytes=cc_bytes(G))),
    (E, "N = 2^30 + 1", dict(N=G + 1, workspace_bytes=HUGE)),
    (E, "workspace one byte short", dict(workspace_bytes=cc_bytes(105) - 1)),
    (E, "N = 1, workspace one byte short", dict(N=1, workspace_bytes=cc_bytes(1) - 1)),
] + _off(E, ("workspace", 8), ("out", 4), ("roots_pred", 2), ("roots_gt", 2)) + [
    (E, "null out and N = 0", dict(out=None, N=0)),
    (E, "N = 0 and workspace short", dict(N=0, workspace_bytes=0)),
    (E, "workspace short and workspace +8", dict(workspace_bytes=0, workspace=P(4) + 8)),
]

E = "rehr_seg_cc_compact_i32"
ROWS += [(E, "valid", {})] + _nulls(E, "roots", "rank", "labels", "count") + [
    (E, "N = 0", dict(N=0)), (E, "N = 2^30", dict(N=G)), (E, "N = 2^30 + 1", dict(N=G + 1)),
] + _off(E, ("roots", 2), ("rank", 2), ("labels", 2), ("count", 4)) + [
    (E, "null rank and N = 0", dict(rank=None, N=0)),
    (E, "N = 0 and count +4", dict(N=0, count=P(4) + 4)),                                  # extent before alignment
]

E = "rehr_order_stats_f32"
R8, R9 = i64(*range(8)), i64(*range(9))
ROWS += [(E, "valid", {}), (E, "valid, one item with a short stride", dict(B=1, item_stride=0,
                                                                          workspace_bytes=order_bytes(1, 3))),
         (E, "valid, 8 ranks", dict(ranks=R8, R=8, workspace_bytes=order_bytes(3, 8)))]
ROWS += _nulls(E, "x", "ranks", "out", "workspace") + [
    (E, "S = 0", dict(S=0)), (E, "item_stride = S - 1", dict(item_stride=104)),
    (E, "B = 0", dict(B=0)), (E, "R = 0", dict(R=0)),
    (E, "B = 65535", dict(B=65535, workspace_bytes=order_bytes(65535, 3))),
    (E, "B = 65536", dict(B=65536, workspace_bytes=HUGE)),
    (E, "R = 9", dict(ranks=R9, R=9, workspace_bytes=HUGE)),
    (E, "S = 2^30", dict(S=G, item_stride=G)), (E, "S = 2^30 + 1", dict(S=G + 1, item_stride=G + 1)),
    (E, "rank -1", dict(ranks=i64(0, -1, 104))), (E, "rank S", dict(ranks=i64(0, 52, 105))),
    (E, "workspace one byte short", dict(workspace_bytes=order_bytes(3, 3) - 1)),
    (E, "B = 65535, workspace one byte short", dict(B=65535, workspace_bytes=order_bytes(65535, 3) - 1)),
] + _off(E, ("workspace", 8), ("x", 2), ("out", 2)) + [
    (E, "S = 0 and B = 65536", dict(S=0, B=65536)),                                        # EINVAL before ENOSUP
    (E, "B = 65536 and rank S", dict(B=65536, ranks=i64(0, 52, 105))),
    (E, "S = 2^30 + 1 and workspace short", dict(S=G + 1, item_stride=G + 1, workspace_bytes=0)),
    (E, "rank S and workspace short", dict(ranks=i64(105, 0, 0), workspace_bytes=0)),
    (E, "workspace short and x +2", dict(workspace_bytes=0, x=P(1) + 2)),
]

E = "rehr_percentile_f64"
ROWS += [(E, "valid", {}), (E, "valid, strictly positive", dict(strictly_positive=1)),
         (E, "valid, t just below 1", dict(t=f64(0.0, 1.0 - 2.0 ** -53)))]
ROWS += _nulls(E, "stats", "t", "out") + [
    (E, "B = 0", dict(B=0)), (E, "Q = 0", dict(Q=0)),
    (E, "Q = 4", dict(Q=4, t=f64(0.0, 0.25, 0.5, 0.75))), (E, "Q = 5", dict(Q=5, t=f64(0.0, 0.2, 0.4, 0.6, 0.8))),
    (E, "t = 1", dict(t=f64(0.25, 1.0))), (E, "t < 0", dict(t=f64(-0.125, 0.5))), (E, "t NaN", dict(t=f64(NAN, 0.5))),
] + _off(E, ("stats", 2), ("out", 4)) + [
    (E, "Q = 5 and stats +2", dict(Q=5, t=f64(0.0, 0.2, 0.4, 0.6, 0.8), stats=P(1) + 2)),   # extent before alignment
    (E, "null out and Q = 5", dict(out=None, Q=5, t=f64(0.0, 0.2, 0.4, 0.6, 0.8))),
    (E, "out +4 and t = 1", dict(out=P(2) + 4, t=f64(1.0, 0.5))),
]

E = "rehr_intensity_apply_f32"
ROWS += [(E, "valid", {}), (E, "valid, zero-one", dict(mode=1)), (E, "valid, in place", dict(y=P(1))),
         (E, "valid, one item with short strides", dict(B=1, x_stride=0, y_stride=0))]
ROWS += _nulls(E, "x", "y", "bounds") + [
    (E, "B = 0", dict(B=0)), (E, "S = 0", dict(S=0)), (E, "mode 2", dict(mode=2)),
    (E, "bounds_stride = 1", dict(bounds_stride=1)),
    (E, "x_stride = S - 1", dict(x_stride=104)), (E, "y_stride = S - 1", dict(y_stride=104)),
    (E, "B = 65535", dict(B=65535)), (E, "B = 65536", dict(B=65536)),
    (E, "S = 2^30", dict(S=G, x_stride=G, y_stride=G)), (E, "S = 2^30 + 1", dict(S=G + 1, x_stride=G + 1, y_stride=G + 1)),
] + _off(E, ("x", 2), ("y", 2), ("bounds", 4), ("x", 4)) + [                            # 4 bytes; 16 only picks the loop
    (E, "mode 2 and B = 65536", dict(mode=2, B=65536)),                                    # EINVAL before ENOSUP
    (E, "B = 65536 and x +2", dict(B=65536, x=P(1) + 2)),                                  # extent before alignment
    (E, "null bounds and B = 65536", dict(bounds=None, B=65536)),
]

E = "rehr_minmax_f32"
ROWS += [(E, "valid", {}), (E, "valid n = 2^31 + 5", dict(n=(1 << 31) + 5))] + _nulls(E, "x", "minmax") + [
    (E, "n = 0", dict(n=0)),
] + _off(E, ("x", 2), ("x", 4), ("x", 8)) + [                                             # 4 bytes; 16 picks the kernel
    (E, "null x and n = 0", dict(x=None, n=0)), (E, "n = 0 and x +2", dict(n=0, x=P(1) + 2)),
]

E = "rehr_sr_window_gather_f32"
ROWS += [(E, "valid", {}), (E, "valid, two channels", dict(C=2)), (E, "valid, two slices", dict(Z=2, b=1))]
ROWS += _nulls(E, "vol", "out") + [
    (E, "X = 0", dict(X=0)), (E, "Z = 1", dict(Z=1, b=1)), (E, "C = 3", dict(C=3)), (E, "w0 = -1", dict(w0=-1)),
    (E, "b = 0", dict(b=0)), (E, "w0 + b = Z - 1", dict(w0=3)), (E, "w0 + b = Z", dict(w0=4)),
    (E, "Xp < X", dict(X=17)), (E, "Xp = 24", dict(Xp=24)), (E, "Yp = 8", dict(Yp=8)),
    (E, "X Y Z C = 2^40", dict(X=1 << 15, Y=1 << 15, Z=1 << 10, Xp=1 << 15, Yp=1 << 15, b=1)),
    (E, "X Y Z C just below 2^40", dict(X=1 << 15, Y=1 << 15, Z=1023, Xp=1 << 15, Yp=1 << 15, b=1)),
    (E, "4 b Xp Yp C = 2^40", dict(X=16, Y=16, Z=1 << 12, b=1 << 11, Xp=1 << 14, Yp=1 << 13)),
] + _off(E, ("out", 8), ("vol", 2), ("vol", 4)) + [
    (E, "null out and C = 3", dict(out=None, C=3)), (E, "Yp = 8 and out +8", dict(Yp=8, out=P(2) + 8)),
]

E = "rehr_sr_volume_scatter_f32"
ROWS += [(E, "valid", {}), (E, "valid, no seg", dict(seg=None)), (E, "valid, one channel", dict(C=1, seg=None)),
         (E, "valid, X % 4 != 0", dict(X=13))]
ROWS += _nulls(E, "net", "strides", "in_minmax", "img", "out_minmax") + [
    (E, "b = 0", dict(b=0)), (E, "C = 0", dict(C=0, seg=None)), (E, "n_out = 0", dict(n_out=0)), (E, "w0 = -1", dict(w0=-1)),
    (E, "w0 + b = n_windows", dict(w0=3)), (E, "w0 + b = n_windows + 1", dict(w0=4)),
    (E, "seg with one channel", dict(C=1)), (E, "negative stride", dict(strides=i64(5000, -1, 300, 20, 1))),
    (E, "n_windows n_out X Y = 2^40", dict(n_windows=1 << 10, n_out=1 << 10, X=1 << 10, Y=1 << 10)),
    (E, "2^31 - 32768 blocks", dict(b=65535, n_out=32768, X=1, Y=1, n_windows=65535)),
    (E, "2^31 blocks", dict(b=65536, n_out=32768, X=1, Y=1, n_windows=65536)),
] + _off(E, ("net", 2), ("img", 2), ("img", 8), ("seg", 2)) + [                          # X % 4 == 0: img 16, seg 4
    (E, "X % 4 != 0, img +4", dict(X=13, img=P(3) + 4)), (E, "X % 4 != 0, seg +1", dict(X=13, seg=P(4) + 1)),
    (E, "null net and b = 0", dict(net=None, b=0)),
    (E, "negative stride and net +2", dict(strides=i64(5000, 1000, 300, 20, -1), net=P(1) + 2)),
]

E = "rehr_stage2_prep_f32"
ROWS += [(E, "valid", {}), (E, "valid, P % 4 != 0", dict(P=157)), (E, "valid, 9 taps", dict(L=9)),
         (E, "valid, 17 taps", dict(L=17))]
ROWS += _nulls(E, "img", "minmax", "taps", "out") + [
    (E, "L = 0", dict(L=0)), (E, "X = 0", dict(X=0)), (E, "P = 0", dict(P=0)),
    (E, "X P = 2^40", dict(X=1 << 20, P=1 << 20)), (E, "X P just below 2^40", dict(X=(1 << 20) - 1, P=1 << 20)),
    (E, "L = 32", dict(L=32)), (E, "L = 33", dict(L=33)), (E, "in place", dict(out=P(1))),
    (E, "65535 chunks", dict(X=65535 * 64, P=4)), (E, "65536 chunks", dict(X=65535 * 64 + 1, P=4)),
] + _off(E, ("img", 2), ("out", 2), ("img", 4), ("out", 8)) + [                          # 4 bytes; 16 picks the kernel
    (E, "L = 33 and in place", dict(L=33, out=P(1))),                                      # ENOSUP before the aliasing check
    (E, "L = 0 and 65536 chunks", dict(L=0, X=65535 * 64 + 1, P=4)),
    (E, "null taps and L = 33", dict(taps=None, L=33)),
]

E = "rehr_stage2_unc_u8_f32"
ROWS += [(E, "valid", {})] + _nulls(E, "u", "minmax", "out") + [(E, "n = 0", dict(n=0))]
ROWS += _off(E, ("u", 2), ("u", 4), ("out", 1)) + [                                       # u 4 bytes; the rest picks the kernel
    (E, "null out and n = 0", dict(out=None, n=0)), (E, "n = 0 and u +2", dict(n=0, u=P(1) + 2)),
]

E = "rehr_zoom_depth_f32"
ROWS += [(E, "valid", {}), (E, "valid, image only", dict(C=1, nn=None, label=None))]
ROWS += _nulls(E, "vol", "idx", "w", "img") + [
    (E, "two channels without nn", dict(nn=None)), (E, "two channels without label", dict(label=None)),
    (E, "lines = 0", dict(lines=0)), (E, "n = 0", dict(n=0)), (E, "Z = 0", dict(Z=0)), (E, "C = 3", dict(C=3)),
    (E, "lines n C = 2^40", dict(lines=1 << 38, n=2, Z=1)), (E, "lines Z = 2^40", dict(lines=1 << 36, n=2)),
    (E, "n = 283", dict(n=283)), (E, "n = 284", dict(n=284)),
    (E, "Z = 2^22 - 1", dict(Z=(1 << 22) - 1)), (E, "Z = 2^22", dict(Z=1 << 22)),
    (E, "2^31 - 1 blocks", dict(lines=0x7fffffff * 256, n=1, C=1, Z=1, nn=None, label=None)),
    (E, "2^31 blocks", dict(lines=0x7fffffff * 256 + 1, n=1, C=1, Z=1, nn=None, label=None)),
] + _off(E, ("vol", 2), ("img", 2), ("idx", 2), ("nn", 2), ("w", 4), ("vol", 8), ("label", 1)) + [
    (E, "n = 284 and vol +2", dict(n=284, vol=P(1) + 2)),                                  # alignment before the extent
    (E, "n = 284 and lines Z = 2^40", dict(n=284, lines=1 << 36)),
    (E, "null w and n = 284", dict(w=None, n=284)),
    (E, "w +4 and Z = 2^22", dict(w=P(3) + 4, Z=1 << 22)),
]

E = "rehr_bspline_prefilter_axis_f64acc_f32"
ROWS += [(E, "valid", {}), (E, "valid, last axis", dict(inner=1))] + _nulls(E, "x", "y") + [
    (E, "in place", dict(y=P(1))), (E, "outer = 0", dict(outer=0)), (E, "n = 0", dict(n=0)), (E, "inner = 0", dict(inner=0)),
    (E, "outer = 2^40", dict(outer=1 << 40, n=1, inner=1)), (E, "outer inner = 2^40", dict(outer=1 << 20, inner=1 << 20, n=1)),
    (E, "outer inner n = 2^40", dict(outer=1 << 19, inner=1 << 20, n=2)),
    (E, "n = 283", dict(n=283)), (E, "n = 284", dict(n=284)), (E, "n = 283, last axis", dict(n=283, inner=1)),
    (E, "last axis, 2^31 - 1 blocks", dict(outer=0x7fffffff * 256, n=1, inner=1)),
    (E, "last axis, 2^31 blocks", dict(outer=0x7fffffff * 256 + 1, n=1, inner=1)),
    (E, "2^31 - 1 blocks", dict(outer=0x7fffffff * 128, n=1, inner=2)),
    (E, "2^31 blocks", dict(outer=0x7fffffff * 128 + 1, n=1, inner=2)),
] + _off(E, ("x", 2), ("y", 2), ("x", 4)) + [
    (E, "n = 284 and x +2", dict(n=284, x=P(1) + 2)),                                      # alignment before the extent
    (E, "n = 284 and outer = 2^40", dict(n=284, outer=1 << 40)),
    (E, "in place and n = 284", dict(y=P(1), n=284)),
]

E = "rehr_blur_to_slices_f32"
ROWS += [(E, "valid", {}), (E, "valid, axis 1", dict(axis=1)), (E, "valid, B % 4 == 0", dict(Y=12))]
ROWS += _nulls(E, "img", "taps", "out") + [
    (E, "in place", dict(out=P(1))), (E, "L = 0", dict(L=0)), (E, "X = 0", dict(X=0)), (E, "axis 2", dict(axis=2)),
    (E, "X Y Z = 2^40", dict(X=1 << 14, Y=1 << 13, Z=1 << 13)),
    (E, "X Y Z just below 2^40", dict(X=(1 << 14) - 1, Y=1 << 13, Z=1 << 13)),
    (E, "L = 32", dict(L=32)), (E, "L = 33", dict(L=33)),
    (E, "65535 chunks", dict(X=65535 * 64, Y=1, Z=1)), (E, "65536 chunks", dict(X=65535 * 64 + 1, Y=1, Z=1)),
    (E, "65535 z tiles", dict(X=1, Y=1, Z=65535 * 64)), (E, "65536 z tiles", dict(X=1, Y=1, Z=65535 * 64 + 1)),
] + _off(E, ("img", 2), ("out", 2), ("taps", 2), ("out", 8)) + [
    (E, "L = 33 and taps +2", dict(L=33, taps=P(2) + 2)),                                  # alignment before the extent
    (E, "L = 33 and axis 2", dict(L=33, axis=2)),
    (E, "null img and L = 33", dict(img=None, L=33)),
]

NOSEG = dict(slog=None, ls=None, stgt=None, gs=None)
for E in ("rehr_sr_metrics_f32", "rehr_sr_metrics_bf16"):
    ROWS += [(E, "valid", {}), (E, "valid, no segmentation pair", NOSEG),
             (E, "valid 1x1x11x11", dict(N=1, D=1, H=11, W=11, workspace_bytes=tile_bytes(1, 6))),
             (E, "valid, data_range inf", dict(data_range=INF))]
    ROWS += _nulls(E, "pred", "ps", "tgt", "ts", "stats", "workspace") + [
        (E, "seg_logits without seg_target", dict(stgt=None)), (E, "seg_target without seg_logits", dict(slog=None)),
        (E, "seg pair without logits strides", dict(ls=None)), (E, "seg pair without target strides", dict(gs=None)),
        (E, "data_range 0", dict(data_range=0.0)), (E, "data_range NaN", dict(data_range=NAN)),
        (E, "N = 0", dict(N=0)), (E, "W = -1", dict(W=-1)),
        (E, "H = 10", dict(H=10)), (E, "W = 10", dict(W=10)),
        (E, "2^31 - 1 tiles", dict(N=0x7fffffff, D=1, workspace_bytes=HUGE)),
        (E, "2^31 + 1 tiles", dict(N=0x7fffffff // 3 + 1, workspace_bytes=HUGE)),
        (E, "workspace one byte short", dict(workspace_bytes=tile_bytes(6, 6) - 1)),
        (E, "negative stride", dict(ts=i64(1000, 300, 20, -1))),
        (E, "negative seg stride", dict(gs=i64(-1000, 300, 20, 1))),
    ] + _off(E, ("workspace", 4), ("workspace", 8), ("stats", 4)) + [
        (E, "H = 10 and workspace short", dict(H=10, workspace_bytes=0)),                  # geometry before the workspace
        (E, "data_range 0 and H = 10", dict(data_range=0.0, H=10)),                       # EINVAL before ENOSUP
        (E, "workspace short and negative stride", dict(workspace_bytes=0, ps=i64(-1, 300, 20, 1))),
        (E, "null stats and H = 10", dict(stats=None, H=10)),
    ]
ROWS += _off("rehr_sr_metrics_bf16", ("pred", 1), ("slog", 1), ("pred", 2)) + [
    ("rehr_sr_metrics_bf16", "pred +1 and H = 10", dict(pred=P(1) + 1, H=10)),
    ("rehr_sr_metrics_bf16", "pred +1 and null tgt", dict(pred=P(1) + 1, tgt=None)),
]

E = "rehr_structure_loss_fwd_f32"
ROWS += [(E, "valid", {}), (E, "valid, no fields", dict(fields=None)),
         (E, "valid 1x1x1x11x11", dict(N=1, C=1, D=1, H=11, W=11, workspace_bytes=tile_bytes(1, 4))),
         (E, "valid, H = 10 without the SSIM term", dict(H=10, ssim=0.0)),
         (E, "valid, all weights 0", dict(l1=0.0, l2=0.0, ssim=0.0, sobel=0.0))]
ROWS += _nulls(E, "input", "istr", "target", "tstr", "stats", "loss", "workspace") + [
    (E, "data_range 0", dict(data_range=0.0)), (E, "data_range NaN", dict(data_range=NAN)),
    (E, "data_range inf", dict(data_range=INF)), (E, "weight NaN", dict(l2=NAN)), (E, "weight inf", dict(sobel=INF)),
    (E, "N = 0", dict(N=0)), (E, "C = -1", dict(C=-1)), (E, "H = 10", dict(H=10)), (E, "W = 10", dict(W=10)),
    (E, "2^31 - 1 tiles", dict(N=0x7fffffff, C=1, D=1, workspace_bytes=HUGE)),
    (E, "2^31 + 4 tiles", dict(N=0x7fffffff // 6 + 1, workspace_bytes=HUGE)),
    (E, "workspace one byte short", dict(workspace_bytes=tile_bytes(12, 4) - 1)),
    (E, "negative stride", dict(istr=i64(5000, 1000, 300, -20, 1))),
] + _off(E, ("workspace", 4), ("workspace", 8), ("stats", 4), ("loss", 2), ("fields", 2)) + [
    (E, "H = 10 and workspace short", dict(H=10, workspace_bytes=0)),                      # geometry before the workspace
    (E, "data_range 0 and H = 10", dict(data_range=0.0, H=10)),                           # EINVAL before ENOSUP
    (E, "weight NaN and H = 10", dict(l1=NAN, H=10)),
    (E, "null loss and N = 0", dict(loss=None, N=0)),
    (E, "workspace short and stats +4", dict(workspace_bytes=0, stats=P(3) + 4)),
]

E = "rehr_structure_loss_bwd_f32"
ROWS += [(E, "valid", {}), (E, "valid, no SSIM term and no fields", dict(ssim=0.0, fields=None)),
         (E, "valid, stride 0 on an axis of extent 1", dict(N=1, dstr=i64(0, 1000, 300, 20, 1)))]
ROWS += _nulls(E, "input", "istr", "target", "tstr", "dinput", "dstr", "grad_output") + [
    (E, "SSIM term without fields", dict(fields=None)),
    (E, "weight NaN", dict(ssim=NAN)), (E, "N = 0", dict(N=0)), (E, "H = 10", dict(H=10)),
    (E, "H = 10 without the SSIM term", dict(H=10, ssim=0.0)),
    (E, "2^31 + 4 tiles", dict(N=0x7fffffff // 6 + 1)),
    (E, "d input stride 0", dict(dstr=i64(5000, 0, 300, 20, 1))),
    (E, "negative d input stride", dict(dstr=i64(5000, 1000, 300, 20, -1))),
] + _off(E, ("fields", 2), ("grad_output", 2)) + [
    (E, "H = 10 and no fields", dict(H=10, fields=None)),                                  # geometry before the fields
    (E, "weight NaN and H = 10", dict(l1=NAN, H=10)),                                      # EINVAL before ENOSUP
    (E, "null grad_output and H = 10", dict(grad_output=None, H=10)),
    (E, "H = 10 and d input stride 0", dict(H=10, dstr=i64(5000, 1000, 0, 20, 1))),
]

# (size query, arguments): invalid and unsupported extents, then valid ones -- among them voxel counts that are no
# multiple of 4 or 16, where the padding between segments matters
QUERIES = [
    ("rehr_seg_surface_workspace_bytes", a) for a in (
        (0, 5, 7), (3, -1, 7), (2049, 1, 1), (1, 1, 2049), (2048, 2048, 257),
        (3, 5, 7), (2, 16, 16), (1, 1, 1), (7, 3, 1), (5, 9, 11), (16, 320, 384), (1, 2048, 1), (2048, 2048, 256))
] + [
    ("rehr_seg_cc_workspace_bytes", a) for a in (
        (0, 5, 7), (3, -1, 7), (1024, 1024, 1025), (65536, 32768, 1),
        (3, 5, 7), (2, 16, 16), (1, 1, 1), (7, 3, 1), (5, 9, 11), (16, 320, 384), (1024, 1024, 1024))
] + [
    ("rehr_order_stats_workspace_bytes", a) for a in (
        (0, 1), (1, 0), (0, 9), (65536, 1), (1, 9),
        (1, 1), (3, 3), (2, 8), (5, 2), (7, 1), (1, 8), (65535, 3), (65535, 8))
] + [
    ("rehr_sr_metrics_workspace_bytes", a) for a in (
        (0, 1, 11, 11), (1, 0, 11, 11), (1, 1, 10, 11), (1, 1, 11, 10), (0x7fffffff // 3 + 1, 3, 12, 13),
        (1, 1, 11, 11), (2, 3, 12, 13), (1, 1, 32, 32), (1, 1, 33, 33), (3, 5, 64, 65), (1, 16, 320, 384), (2, 1, 11, 43),
        (0x7fffffff, 1, 12, 13))
] + [
    ("rehr_structure_loss_workspace_bytes", a) for a in (
        (0, 1, 1, 11, 11), (1, 1, 1, 11, 0), (0x7fffffff // 6 + 1, 2, 3, 12, 13), (1, 65536, 65536, 12, 13),
        (1, 1, 1, 11, 11), (2, 2, 3, 12, 13), (1, 1, 1, 5, 5), (1, 3, 2, 33, 65), (2, 1, 16, 320, 384), (3, 3, 3, 3, 3),
        (0x7fffffff, 1, 1, 12, 13))
]


def row_name(entry, label):
    return f"{entry}: {label}"


def query_name(entry, args):
    return f"{entry}{tuple(args)}"


def record(lib, launches):
    """What `lib` answers to the table: {"queries": {name: bytes or code}, "launches": {name: code}}; the launch half
    only where asked for (never where there is a device)."""
    rec = {"queries": {query_name(e, a): int(getattr(lib, e)(*a)) for e, a in QUERIES}}
    if launches:
        rec["launches"] = {row_name(e, label): int(getattr(lib, e)(*call_args(e, over))) for e, label, over in ROWS}
    return rec


EINVAL, ENOSUP, EHIP = -1, -2, -3


def table_condition(launches):
    """The table is not one-sided: every launch entry point is accepted at least once and refused at least once, every
    one that documents an extent limit meets it, and there are at least 150 rows.  -> list of complaints."""
    bad = []
    names = [row_name(e, label) for e, label, _ in ROWS]
    if len(set(names)) != len(names):
        bad.append("row names are not unique")
    if len(names) < 150:
        bad.append(f"only {len(names)} rows")
    if set(names) != set(launches):
        bad.append("the recorded rows are not the table's rows")
        return bad
    by_entry = {}
    for e, label, _ in ROWS:
        by_entry.setdefault(e, set()).add(launches[row_name(e, label)])
    if len(by_entry) != 23 or set(by_entry) != set(CALLS):
        bad.append(f"{len(by_entry)} launch entry points, not 23")
    for e, codes in sorted(by_entry.items()):
        want = {EHIP, EINVAL} | ({ENOSUP} if e in HAS_EXTENT_LIMIT else set())
        if not want <= codes:
            bad.append(f"{e}: no row returned {sorted(want - codes)}")
        if not codes <= {EHIP, EINVAL, ENOSUP}:
            bad.append(f"{e}: unexpected codes {sorted(codes)}")
    return bad
