"""The cases of tests/test_conv_route_gpu.py: one public convolution call each, small enough to run in milliseconds.

A case is a dict.  `op` names the public function, `shape` the activation on the input side (4-D or 5-D, channels last), `co` the
output channels, k / stride / pad / dil the window as the public functions take them.  Flags: res, mask, relu, inference, pool,
out ("dense" / "slice"), acc (the parameter already holds a gradient), images ("active": a WeightImages with this weight is
ACTIVE_IMAGES, "idle": registered but ACTIVE_IMAGES is None), profile (PROFILE = []), deferred (DEFERRED_WGRADS = []), env
(environment switches), attrs (module switches of hipops).  tests/golden/conv_routes.json holds these dicts next to what the parent
commit launched for them."""


def _c(id, op, shape, co, k=3, stride=1, pad=1, **kw):
    return dict(id=id, op=op, shape=list(shape), co=co, k=k, stride=stride, pad=pad, **kw)


def _three(id, shape, co, k=3, stride=1, pad=1, **kw):
    return [_c(id + "_" + op, op, shape, co, k, stride, pad, **kw) for op in ("fwd", "dgrad", "wgrad")]


F32 = {"MI_CONV_ARITH": "f32"}
G = (2, 6, 6, 6, 16)                  # generic
DIL = dict(k=(3, 3, 3), pad=(1, 4, 4), dil=(1, 4, 4))
CUBE = (4, 2, 2, 2, 256)
L1 = (4, 8, 8, 8, 64)
S2 = (32, 8, 8, 8, 64)
S2_NO = (32, 16, 16, 16, 64)
ST3 = (2, 12, 20, 1)
P2D = (2, 18, 18, 128)
ST2D = (2, 21, 37, 1)
K1 = (2, 16, 32, 16)                  # -> 32: d32 kind 1; -> 64 from 32 channels: kind 3
K3 = (2, 16, 32, 32)
K2 = (1, 6, 32, 32, 32)               # the dilated 3-D head: kind 2
K4 = (1, 16, 32, 32)                  # 1 x 1: kind 4
SK1 = (1, 8, 16, 16)                  # 1 x 1 from 16 channels: conv_d32 declines, conv_smallk with one tap
SK3 = (1, 4, 8, 16, 32)               # (3, 1, 1): conv_smallk with three taps

CASES = (
    # ---- the generic entries -----------------------------------------------------------------------------------------
    _three("generic", G, 32)
    + [_c("generic_fwd_res_relu", "fwd", G, 32, res=True, relu=True),
       _c("generic_dgrad_res_mask", "dgrad", G, 32, res=True, mask=True),
       _c("generic_wgrad_acc", "wgrad", G, 32, acc=True),
       _c("generic_wgrad_deferred", "wgrad", G, 32, deferred=True)]
    + _three("dilated", (1, 6, 20, 24, 32), 32, **DIL)
    + _three("generic4d", (2, 10, 12, 16), 32)
    # ---- families the library picks behind the generic entry ------------------------------------------------------------
    + _three("lib_direct3", L1, 64)
    + [_c("lib_direct3_wgrad_deferred", "wgrad", L1, 64, deferred=True)]
    + _three("lib_direct3s", (4, 4, 4, 4, 128), 128)
    + [_c("lib_stem_fwd", "fwd", (1, 8, 8, 16, 1), 64, 7, 2, 3), _c("lib_stem_wgrad", "wgrad", (1, 8, 8, 16, 1), 64, 7, 2, 3)]
    # ---- cube2 in one launch ----------------------------------------------------------------------------------------------
    + _three("cube2", CUBE, 256)
    + [_c("cube2_fwd_res_relu", "fwd", CUBE, 256, res=True, relu=True),
       _c("cube2_fwd_reduce", "fwd", CUBE, 256, env={"MI_CUBE2_REDUCE": "1"}),
       _c("cube2_dgrad_reduce", "dgrad", CUBE, 256, env={"MI_CUBE2_REDUCE": "1"}),
       _c("cube2_fwd_f32", "fwd", CUBE, 256, env=F32), _c("cube2_dgrad_f32", "dgrad", CUBE, 256, env=F32),
       _c("cube2_fwd_unit_dil", "fwd", CUBE, 256, dil=(1, 1, 1)), _c("cube2_dgrad_unit_dil", "dgrad", CUBE, 256, dil=(1, 1, 1))]
    # ---- the pre-cut direct image -----------------------------------------------------------------------------------------
    + [_c("direct_fwd", "fwd", L1, 64, images="active"), _c("direct_dgrad", "dgrad", L1, 64, images="active"),
       _c("direct_fwd_res_relu", "fwd", L1, 64, images="active", res=True, relu=True),
       _c("direct_dgrad_res_mask", "dgrad", L1, 64, images="active", res=True, mask=True),
       _c("direct_fwd_profile", "fwd", L1, 64, images="active", profile=True),
       _c("direct_dgrad_profile", "dgrad", L1, 64, images="active", profile=True),
       _c("direct_fwd_idle", "fwd", L1, 64, images="idle"), _c("direct_dgrad_idle", "dgrad", L1, 64, images="idle"),
       _c("direct_fwd_f32", "fwd", L1, 64, images="active", env=F32),
       _c("direct_fwd_other_shape", "fwd", (2, 6, 6, 6, 64), 64, images="active")]
    # ---- the stride-2 block fronts ------------------------------------------------------------------------------------------
    + [_c("s2_fwd", "s2_fwd", S2, 128, 3, 2, 1), _c("s2_dgrad", "s2_dgrad", S2, 128, 3, 2, 1),
       _c("s2_dgrad_res_mask", "s2_dgrad", S2, 128, 3, 2, 1, res=True, mask=True),
       _c("s2_fwd_image", "s2_fwd", S2, 128, 3, 2, 1, images="active"), _c("s2_dgrad_image", "s2_dgrad", S2, 128, 3, 2, 1, images="active"),
       _c("s2_fwd_image_profile", "s2_fwd", S2, 128, 3, 2, 1, images="active", profile=True),
       _c("s2_fwd_declined", "s2_fwd", S2_NO, 128, 3, 2, 1), _c("s2_dgrad_declined", "s2_dgrad", S2_NO, 128, 3, 2, 1)]
    # ---- Conv2d(1, co, 3, padding 1) ------------------------------------------------------------------------------------------
    + [_c("stem3_fwd", "fwd", ST3, 16), _c("stem3_wgrad", "wgrad", ST3, 16), _c("stem3_wgrad_acc", "wgrad", ST3, 16, acc=True),
       _c("stem3_fwd_off", "fwd", ST3, 16, env={"MI_NO_P2D": "1"}), _c("stem3_wgrad_off", "wgrad", ST3, 16, env={"MI_NO_P2D": "1"}),
       _c("stem3_fwd_co48", "fwd", ST3, 48), _c("stem3_wgrad_co48", "wgrad", ST3, 48),    # 256 % (48 / 4) != 0
       _c("stem3_fwd_relu", "fwd", ST3, 16, relu=True)]
    # ---- the 2-D C -> C layers ---------------------------------------------------------------------------------------------
    + _three("p2d", P2D, 128)
    + [_c("p2d_fwd_res_relu", "fwd", P2D, 128, res=True, relu=True), _c("p2d_dgrad_res_mask", "dgrad", P2D, 128, res=True, mask=True),
       _c("p2d_fwd_image", "fwd", P2D, 128, images="active"), _c("p2d_dgrad_image", "dgrad", P2D, 128, images="active"),
       _c("p2d_wgrad_acc", "wgrad", P2D, 128, acc=True)]
    + _three("p2d_off", P2D, 128, env={"MI_NO_P2D": "1"})
    + [_c("p2d_wgrad_switch", "wgrad", P2D, 128, env={"MI_NO_P2D_WGRAD": "1"})]
    + _three("p2d_f32", P2D, 128, env=F32)
    # ---- the detector's first layer -------------------------------------------------------------------------------------------
    + [_c("stem2d", "bias_fwd", ST2D, 16, 7, 2, 3, relu=True), _c("stem2d_off", "bias_fwd", ST2D, 16, 7, 2, 3, relu=True, env={"MI_NO_STEM2D": "1"}),
       _c("stem2d_out", "bias_fwd", ST2D, 16, 7, 2, 3, out="dense")]
    # ---- inference: conv_d32 kinds 1 - 4, conv_smallk with 1 and 3 taps --------------------------------------------------------
    + [_c("%s_%s%s" % (name, op, "" if smallk else "_nosmallk"), op, shape, co, k, 1, pad, relu=True, inference=True,
          attrs={"SMALLK": smallk}, **kw)
       for name, shape, co, k, pad, kw in (("kind1", K1, 32, 3, 1, {}), ("kind3", K3, 64, 3, 1, {}), ("kind4", K4, 32, 1, 0, {}),
                                           ("smallk1", SK1, 32, 1, 0, {}), ("smallk3", SK3, 32, (3, 1, 1), (1, 0, 0), {}),
                                           ("kind2", K2, 32, (3, 3, 3), (1, 4, 4), {"dil": (1, 4, 4)}))
       for op in ("fwd", "bias_fwd") if not (name == "kind2" and op == "bias_fwd") for smallk in (True, False)]
    + [_c("kind1_fwd_training", "fwd", K1, 32), _c("kind1_fwd_inference_res", "fwd", K1, 32, inference=True, res=True),
       _c("kind4_fwd_inference_res", "fwd", K4, 32, 1, 1, 0, inference=True, res=True),
       _c("kind1_fwd_f32", "fwd", K1, 32, inference=True, env=F32), _c("kind1_bias_out", "bias_fwd", K1, 32, out="dense"),
       _c("kind4_bias_out", "bias_fwd", K4, 32, 1, 1, 0, out="dense"), _c("smallk1_bias_out", "bias_fwd", SK1, 32, 1, 1, 0, out="dense"),
       _c("generic_bias", "bias_fwd", (2, 10, 12, 16), 48, relu=True), _c("generic_bias_out", "bias_fwd", (2, 10, 12, 16), 48, out="dense")]
    # ---- ... with the pooled second output --------------------------------------------------------------------------------------
    + [_c("%s_pool%s%s" % (name, "_fused" if fused else "_unfused", "_" + out if out else ""), "bias_fwd", shape, co, relu=True, pool=True,
          out=out, attrs={"POOL_FUSED": fused})
       for name, shape, co in (("kind1", K1, 32), ("kind3", K3, 64)) for fused in (True, False) for out in (None, "slice")]
    + [_c("kind4_pool", "bias_fwd", K4, 32, 1, 1, 0, pool=True), _c("kind1_pool_profile", "bias_fwd", K1, 32, pool=True, profile=True),
       _c("generic_pool", "bias_fwd", (2, 10, 12, 16), 48, pool=True)]
    # ---- BatchNorm folding and the concatenation paths ---------------------------------------------------------------------------
    + [_c("conv_bn_folded", "conv_bn", K1, 32, relu=True), _c("conv_bn_folded_pool", "conv_bn", K1, 32, relu=True, pool=True),
       _c("conv_bn_folded_pool_slice", "conv_bn", K1, 32, relu=True, pool=True, out="slice"),
       _c("conv_bn_unfolded", "conv_bn", K1, 32, relu=True, attrs={"FOLD_EVAL_BN": False}),
       _c("conv_bn_unfolded_pool", "conv_bn", K1, 32, relu=True, pool=True, attrs={"FOLD_EVAL_BN": False}),
       _c("skip_ok", "skip_ok", K1, 32), _c("skip_ok_64", "skip_ok", K3, 64), _c("skip_no_width", "skip_ok", (2, 16, 24, 16), 32),
       _c("skip_no_channels", "skip_ok", K1, 48), _c("skip_no_f32", "skip_ok", K1, 32, env=F32),
       _c("skip_no_pool_unfused", "skip_ok", K1, 32, attrs={"POOL_FUSED": False}),
       _c("upconv_cat", "upconv", (2, 8, 16, 64), 32, cat=True), _c("upconv_fused", "upconv", (2, 8, 16, 64), 32),
       _c("upconv_tail", "upconv", (2, 8, 16, 64), 32, attrs={"UPCONV_FUSED": False}),
       _c("upconv_tail_ragged", "upconv", (2, 7, 9, 64), 32), _c("upconv_unfolded", "upconv", (2, 8, 16, 64), 32, attrs={"FOLD_EVAL_BN": False})]
    # ---- bench.py's roofline pass ---------------------------------------------------------------------------------------------
    + [_c("generic_fwd_profile", "fwd", G, 32, profile=True), _c("generic_wgrad_profile", "wgrad", G, 32, profile=True),
       _c("lib_direct3_wgrad_profile", "wgrad", L1, 64, profile=True), _c("cube2_dgrad_profile", "dgrad", CUBE, 256, profile=True),
       _c("p2d_fwd_profile", "fwd", P2D, 128, profile=True), _c("stem3_wgrad_profile", "wgrad", ST3, 16, profile=True),
       _c("kind3_bias_profile", "bias_fwd", K3, 64, relu=True, profile=True), _c("smallk3_fwd_profile", "fwd", SK3, 32, (3, 1, 1), 1, (1, 0, 0),
                                                                                    inference=True, profile=True),
       _c("s2_dgrad_profile", "s2_dgrad", S2, 128, 3, 2, 1, profile=True)]
)

assert len({c["id"] for c in CASES}) == len(CASES)
