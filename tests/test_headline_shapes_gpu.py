"""Every kernel launch of the headline step -- one critic + one generator update at level 5 (2x128x128), batch 64: the critic on
192 images [real | fake | interpolated], its tangent pass on 64, the generator on 64 -- run on its own at EXACTLY the shape and
flags the step launches it with, on seeded random inputs, and compared element by element with a float64 host reference of the
same operation (F.conv2d / F.conv_transpose2d / F.avg_pool2d / F.interpolate / autograd, and the restatements of the per-op
tests).  The per-op tests run these kernels at 1-7 images; the routing and tiling decisions that depend on the batch (the
tile-group data gradient from N (H/8) (W/16) >= 128, the small-map kernel up to 8192 pixels, the strip kernel's grid and
persistent walk, the weight gradients' slabs and grouped sweeps) only take these paths at the benchmark's size.

`LAUNCHES` and the two deferred weight-gradient sweeps are the routing census (tests/routing_census.py) of that step, committed:
`test_headline_step_launches_are_all_covered` runs the step and fails when routing sends a launch that is not in the list, so a
new shape is covered before it ships.  Forward and data-gradient launches compare every image (the float64 reference is
computed in slices of images); the weight gradients replay each sweep -- the same layers in the same order into one
`WgradDefer` -- and compare every tensor in full.

Bounds: those of the per-op test of each kernel (test_ops_gpu.py, test_winoups_gpu.py, test_wino_strip_gpu.py,
test_fade_ends_gpu.py, test_smallnet_gpu.py, test_wgrad_rows_gpu.py); for a weight gradient the larger of that bound and twice
plain fp32 PyTorch's own deviation from float64 at the same shape (the rule of golden_util.grad_atol: the reduction length
N H W grows with the batch), which the test measures and prints per layer.

The census, the float64 restatements and the comparisons live in tests/launch_checks.py and do not depend on this configuration;
this file holds the committed lists of level 5 batch 64 and the tests over them."""
import pytest

from launch_checks import _launch, _pn, check_launch, check_sweep, step_census, sweeps_of  # noqa: F401  (_pn: test_poison_gpu.py)
from routing_census import spec

pytestmark = pytest.mark.gpu

LEVEL, BATCH = 5, 64

LAUNCHES = [
    "conv3x3_small x=[64,32,2,2] wpk=[9216] bias=[32] cout=32 ups=False lrelu=True mask_aux=None out=None pool=False pool_out=None",
    "conv3x3_small_pn x_raw=[64,32,2,2] wpk=[36864] bias=[128] cout=128 ups=True save=False",
    "conv3x3_small_pn x_raw=[64,128,4,4] wpk=[147456] bias=[128] cout=128 ups=False save=False",
    "pixelnorm_fwd y=[64,128,4,4]",
    "conv3x3 x=[64,128,4,4] wp=[129024] bias=[112] cout=112 ups=True lrelu=True",
    "pixelnorm_fwd y=[64,112,8,8]",
    "conv3x3 x=[64,112,8,8] wp=None bias=[112] cout=112 ups=False lrelu=True wino=[258048]",
    "upsample2x_fwd x=[64,112,8,8]",
    "conv3x3 x=[64,112,16,16] wp=None bias=[96] cout=96 lrelu=True wino=[229376]",
    "pixelnorm_fwd y=[64,96,16,16]",
    "conv3x3 x=[64,96,16,16] wp=None bias=[96] cout=96 lrelu=True wino=[196608]",
    "upconv3x3 x=[64,96,16,16] wp=[122880] bias=[80] cout=80 lrelu=True pixnorm=True want_y=False",
    "conv3x3 x=[64,80,32,32] wp=None bias=[80] cout=80 lrelu=True wino=[163840]",
    "pixelnorm_fwd y=[64,80,32,32]",
    "upconv3x3 x=[64,80,32,32] wp=[81920] bias=[64] cout=64 lrelu=True pixnorm=True want_y=False",
    "conv3x3 x=[64,64,64,64] wp=None bias=[64] cout=64 ups=False lrelu=True pixnorm=True want_y=False wino=[98304]",
    "winoups3x3_head x=[64,64,64,64] up=[27648] bias=[48] cout=48 hw=[2,48,1,1] hb=[2] mp_out=None",
    "head_pair_from_mp mp=[64,2,128,128] xl=[64,64,64,64] wo=[2,64,1,1] bo=[2] a=0.5 b=0.5 coef=None save=False out=[64,2,128,128]",
    "gp_interp x_real=[64,2,128,128] x_fake=[64,2,128,128] eps=[64,1,1,1] out=[64,2,128,128]",
    "stem_pair x=[192,2,128,128] ws=[48,2,1,1] bs=[48] wo=[64,2,1,1] bo=[64] want_xp=True want_mask=True",
    "conv3x3 x=[192,48,128,128] wp=None bias=[64] cout=64 lrelu=True pool=True wino=[73728] mask_out=True",
    "conv3x3_fade x=[192,64,64,64] wino=[98304] bias=[64] cout=64 mode=1 other=[192,64,64,64] coef=[2]",
    "conv3x3 x=[192,64,64,64] wp=None bias=[80] cout=80 lrelu=True pool=True wino=[131072] mask_out=True",
    "conv3x3 x=[192,80,32,32] wp=None bias=[80] cout=80 lrelu=True wino=[163840]",
    "conv3x3 x=[192,80,32,32] wp=None bias=[96] cout=96 lrelu=True pool=True wino=[163840] mask_out=True",
    "conv3x3 x=[192,96,16,16] wp=None bias=[96] cout=96 lrelu=True wino=[196608]",
    "conv3x3 x=[192,96,16,16] wp=None bias=[112] cout=112 lrelu=True pool=True wino=[221184] mask_out=True",
    "conv3x3 x=[192,112,8,8] wp=None bias=[112] cout=112 lrelu=True wino=[258048]",
    "conv3x3 x=[192,112,8,8] wp=None bias=[128] cout=128 lrelu=True pool=True wino=[258048] mask_out=True",
    "conv3x3_small x=[192,128,4,4] wpk=[147456] bias=[128] cout=128 ups=False lrelu=True mask_aux=None out=None pool=False pool_out=None",
    "conv3x3_small x=[192,128,4,4] wpk=[165888] bias=[144] cout=144 ups=False lrelu=True mask_aux=None out=None pool=True pool_out=None",
    "conv3x3_small x=[192,144,2,2] wpk=[186624] bias=[144] cout=144 ups=False lrelu=True mask_aux=None out=None pool=False pool_out=None",
    "conv3x3_small x=[192,144,2,2] wpk=[207360] bias=[160] cout=160 ups=False lrelu=True mask_aux=None out=None pool=True pool_out=None",
    "conv3x3 x=[192,160,1,1] wp=[230400] bias=[160] cout=160 lrelu=True",
    "linear1_fwd x=[192,160] w=[1,160] b=[1]",
    "linear1_bwd x=[192,160] w=[1,160] gy=[192,1] need_gx=True",
    "lrelu_bwd g=[192,160,1,1] act=[192,160,1,1]",
    "conv3x3 x=[192,160,1,1] wp=[230400] bias=None cout=160",
    "avgpool2_bwd gy=[192,160,1,1] act=[192,160,2,2]",
    "conv3x3_small x=[192,160,2,2] wpk=[207360] bias=None cout=144 ups=False lrelu=False mask_aux=[192,144,2,2] out=None pool=False pool_out=None",
    "conv3x3_small x=[192,144,2,2] wpk=[186624] bias=None cout=144 unpool_aux=[192,144,4,4]",
    "conv3x3_small x=[192,144,4,4] wpk=[165888] bias=None cout=128 ups=False lrelu=False mask_aux=[192,128,4,4] out=None pool=False pool_out=None",
    "conv3x3_small x=[192,128,4,4] wpk=[147456] bias=None cout=128 ups=False lrelu=False mask_aux=None out=None pool=False pool_out=None",
    "avgpool2_bwd gy=[192,128,4,4] act=u8[192,128,4,4]",
    "conv3x3 x=[192,128,8,8] wp=None bias=None cout=112 mask_aux=[192,112,8,8] wino=[294912]",
    "conv3x3 x=[192,112,8,8] wp=None bias=None cout=112 wino=[258048] unpool_mask=u8[192,112,8,8]",
    "conv3x3 x=[192,112,16,16] wp=None bias=None cout=96 mask_aux=[192,96,16,16] wino=[229376]",
    "conv3x3 x=[192,96,16,16] wp=None bias=None cout=96 wino=[196608] unpool_mask=u8[192,96,16,16]",
    "conv3x3 x=[192,96,32,32] wp=None bias=None cout=80 mask_aux=[192,80,32,32] wino=[196608]",
    "conv3x3 x=[192,80,32,32] wp=None bias=None cout=80 wino=[163840] unpool_mask=u8[192,80,32,32]",
    "conv3x3_fade x=[192,80,64,64] wino=[122880] bias=None cout=64 mode=3 other=[192,64,64,64] coef=[2] mask_in=u8[192,64,32,32]",
    "conv3x3 x=[192,64,64,64] wp=None bias=None cout=64 wino=[98304] unpool_mask=u8[192,64,64,64]",
    "conv3x3 x=[192,64,128,128] wp=None bias=None cout=48 mask_aux=u8[192,48,64,64] wino=[65536]",
    "stem_pair_gx gs=[64,48,128,128] ws=[48,2,1,1] go=[64,64,64,64] wo=[64,2,1,1]",
    "sumsq_per_sample g=[64,2,128,128]",
    "gp_apply g=[64,2,128,128] sumsq=[64] factor=10.0 upstream=1.0 out=[64,2,128,128]",
    "stem_pair x=[64,2,128,128] ws=[48,2,1,1] bs=None wo=[64,2,1,1] bo=None h0=[64,48,128,128] xp=[64,2,64,64] o=[64,64,64,64] masked=True",
    "conv3x3 x=[64,48,128,128] wp=None bias=None cout=64 mask_aux=u8[64,64,64,64] pool_out=[64,64,64,64] wino=[73728]",
    "conv3x3_fade x=[64,64,64,64] wino=[98304] bias=None cout=64 mode=2 other=[64,64,64,64] coef=[2] mask_in=u8[64,64,32,32] out=[64,64,64,64]",
    "conv3x3 x=[64,64,64,64] wp=None bias=None cout=80 mask_aux=u8[64,80,32,32] pool_out=[64,80,32,32] wino=[131072]",
    "conv3x3 x=[64,80,32,32] wp=None bias=None cout=80 mask_aux=[64,80,32,32] out=[64,80,32,32] wino=[163840]",
    "conv3x3 x=[64,80,32,32] wp=None bias=None cout=96 mask_aux=u8[64,96,16,16] pool_out=[64,96,16,16] wino=[163840]",
    "conv3x3 x=[64,96,16,16] wp=None bias=None cout=96 mask_aux=[64,96,16,16] out=[64,96,16,16] wino=[196608]",
    "conv3x3 x=[64,96,16,16] wp=None bias=None cout=112 mask_aux=u8[64,112,8,8] pool_out=[64,112,8,8] wino=[221184]",
    "conv3x3 x=[64,112,8,8] wp=None bias=None cout=112 mask_aux=[64,112,8,8] out=[64,112,8,8] wino=[258048]",
    "conv3x3 x=[64,112,8,8] wp=None bias=None cout=128 mask_aux=u8[64,128,4,4] pool_out=[64,128,4,4] wino=[258048]",
    "conv3x3_small x=[64,128,4,4] wpk=[147456] bias=None cout=128 ups=False lrelu=False mask_aux=[64,128,4,4] out=[64,128,4,4] pool=False pool_out=None",
    "conv3x3_small x=[64,128,4,4] wpk=[165888] bias=None cout=144 ups=False lrelu=False mask_aux=[64,144,4,4] out=[64,144,4,4] pool=True pool_out=[64,144,2,2]",
    "conv3x3_small x=[64,144,2,2] wpk=[186624] bias=None cout=144 ups=False lrelu=False mask_aux=[64,144,2,2] out=[64,144,2,2] pool=False pool_out=None",
    "conv3x3_small x=[64,144,2,2] wpk=[207360] bias=None cout=160 ups=False lrelu=False mask_aux=[64,160,2,2] out=[64,160,2,2] pool=True pool_out=[64,160,1,1]",
    "conv3x3 x=[64,160,1,1] wp=[230400] bias=None cout=160 mask_aux=[64,160,1,1] out=[64,160,1,1]",
    "conv1x1_wgrad x=[192,2,128,128] gy=[192,48,128,128] gw=[48,2,1,1] gb=[48] accumulate=False bias_n=128",
    "conv1x1_wgrad x=[192,2,64,64] gy=[192,64,64,64] gw=[64,2,1,1] gb=[64] accumulate=False bias_n=128",
    "linear1_bwd x=[192,160] w=[1,160] gy=[192,1] gw=[1,160] gb=[1] need_gx=False accumulate=False bias_n=128",
    "group_means scores=[192,1] groups=3",
    "conv3x3_small_pn x_raw=[64,32,2,2] wpk=[36864] bias=[128] cout=128 ups=True save=True",
    "conv3x3_small_pn x_raw=[64,128,4,4] wpk=[147456] bias=[128] cout=128 ups=False save=True",
    "head_pair_from_mp mp=[64,2,128,128] xl=[64,64,64,64] wo=[2,64,1,1] bo=[2] a=0.5 b=0.5 coef=None save=True out=None",
    "stem_pair x=[64,2,128,128] ws=[48,2,1,1] bs=[48] wo=[64,2,1,1] bo=[64] want_xp=True want_mask=True",
    "conv3x3 x=[64,48,128,128] wp=None bias=[64] cout=64 lrelu=True pool=True wino=[73728] mask_out=True",
    "conv3x3_fade x=[64,64,64,64] wino=[98304] bias=[64] cout=64 mode=1 other=[64,64,64,64] coef=[2]",
    "conv3x3 x=[64,64,64,64] wp=None bias=[80] cout=80 lrelu=True pool=True wino=[131072] mask_out=True",
    "conv3x3 x=[64,80,32,32] wp=None bias=[96] cout=96 lrelu=True pool=True wino=[163840] mask_out=True",
    "conv3x3 x=[64,96,16,16] wp=None bias=[112] cout=112 lrelu=True pool=True wino=[221184] mask_out=True",
    "conv3x3 x=[64,112,8,8] wp=None bias=[112] cout=112 lrelu=True wino=[258048]",
    "conv3x3 x=[64,112,8,8] wp=None bias=[128] cout=128 lrelu=True pool=True wino=[258048] mask_out=False",
    "conv3x3_small x=[64,128,4,4] wpk=[147456] bias=[128] cout=128 ups=False lrelu=True mask_aux=None out=None pool=False pool_out=None",
    "conv3x3_small x=[64,128,4,4] wpk=[165888] bias=[144] cout=144 ups=False lrelu=True mask_aux=None out=None pool=True pool_out=None",
    "conv3x3_small x=[64,144,2,2] wpk=[186624] bias=[144] cout=144 ups=False lrelu=True mask_aux=None out=None pool=False pool_out=None",
    "conv3x3_small x=[64,144,2,2] wpk=[207360] bias=[160] cout=160 ups=False lrelu=True mask_aux=None out=None pool=True pool_out=None",
    "conv3x3 x=[64,160,1,1] wp=[230400] bias=[160] cout=160 lrelu=True",
    "linear1_fwd x=[64,160] w=[1,160] b=[1]",
    "linear1_bwd x=[64,160] w=[1,160] gy=[64,1] need_gx=True",
    "lrelu_bwd g=[64,160,1,1] act=[64,160,1,1]",
    "conv3x3 x=[64,160,1,1] wp=[230400] bias=None cout=160",
    "avgpool2_bwd gy=[64,160,1,1] act=[64,160,2,2]",
    "conv3x3_small x=[64,160,2,2] wpk=[207360] bias=None cout=144 ups=False lrelu=False mask_aux=[64,144,2,2] out=None pool=False pool_out=None",
    "conv3x3_small x=[64,144,2,2] wpk=[186624] bias=None cout=144 unpool_aux=[64,144,4,4]",
    "conv3x3_small x=[64,144,4,4] wpk=[165888] bias=None cout=128 ups=False lrelu=False mask_aux=[64,128,4,4] out=None pool=False pool_out=None",
    "conv3x3_small x=[64,128,4,4] wpk=[147456] bias=None cout=128 unpool_aux=[64,128,8,8]",
    "conv3x3 x=[64,128,8,8] wp=None bias=None cout=112 mask_aux=[64,112,8,8] wino=[294912]",
    "conv3x3 x=[64,112,8,8] wp=None bias=None cout=112 wino=[258048] unpool_mask=u8[64,112,8,8]",
    "conv3x3 x=[64,112,16,16] wp=None bias=None cout=96 mask_aux=[64,96,16,16] wino=[229376]",
    "conv3x3 x=[64,96,16,16] wp=None bias=None cout=96 wino=[196608] unpool_mask=u8[64,96,16,16]",
    "conv3x3 x=[64,96,32,32] wp=None bias=None cout=80 mask_aux=[64,80,32,32] wino=[196608]",
    "conv3x3 x=[64,80,32,32] wp=None bias=None cout=80 wino=[163840] unpool_mask=u8[64,80,32,32]",
    "conv3x3_fade x=[64,80,64,64] wino=[122880] bias=None cout=64 mode=3 other=[64,64,64,64] coef=[2] mask_in=u8[64,64,32,32]",
    "conv3x3 x=[64,64,64,64] wp=None bias=None cout=64 wino=[98304] unpool_mask=u8[64,64,64,64]",
    "conv3x3 x=[64,64,128,128] wp=None bias=None cout=48 mask_aux=u8[64,48,64,64] wino=[65536]",
    "blend_up_bwd g=[64,2,128,128] a=0.5 b=0.5 coef=None",
    "gen_head_bwd g_mp=[64,2,128,128] mp=[64,2,128,128] w=[2,48,1,1] p=[64,48,128,128] rn=[64,1,128,128] gw=[2,48,1,1] gb=[2] accumulate=False",
    "winoups3x3_dgrad_pn gy=[64,48,128,128] up=[27648] p=[64,64,64,64] rn=[64,1,64,64] cin=64",
    "conv3x3 x=[64,64,64,64] wp=None bias=None cout=64 wino=[98304]",
    "gen_head_bwd g_mp=[64,2,64,64] mp=[64,2,64,64] w=[2,64,1,1] p=[64,64,64,64] rn=[64,1,64,64] gw=[2,64,1,1] gb=[2] accumulate=False g_in=[64,64,64,64]",
    "winoups3x3_dgrad gy=[64,64,64,64] up=[46080] cin=80",
    "pixelnorm_lrelu_bwd gp=[64,80,32,32] y=[64,80,32,32] rn=[64,1,32,32] from_p=True",
    "conv3x3 x=[64,80,32,32] wp=None bias=None cout=80 wino=[163840]",
    "winoups3x3_dgrad gy=[64,80,32,32] up=[69120] cin=96",
    "pixelnorm_lrelu_bwd gp=[64,96,16,16] y=[64,96,16,16] rn=[64,1,16,16] from_p=True",
    "conv3x3 x=[64,96,16,16] wp=None bias=None cout=96 wino=[196608]",
    "conv3x3 x=[64,96,16,16] wp=None bias=None cout=112 wino=[221184]",
    "upsample2x_bwd gy=[64,112,16,16]",
    "pixelnorm_lrelu_bwd gp=[64,112,8,8] y=[64,112,8,8] rn=[64,1,8,8] from_p=True",
    "conv3x3 x=[64,112,8,8] wp=None bias=None cout=112 wino=[258048]",
    "conv3x3 x=[64,112,8,8] wp=None bias=None cout=128 wino=[258048]",
    "upsample2x_bwd gy=[64,128,8,8]",
    "pixelnorm_lrelu_bwd gp=[64,128,4,4] y=[64,128,4,4] rn=[64,1,4,4] from_p=True",
    "conv3x3_small x=[64,128,4,4] wpk=[147456] bias=None cout=128 ups=False lrelu=False mask_aux=None out=None pool=False pool_out=None",
    "conv3x3_small x=[64,128,4,4] wpk=[36864] bias=None cout=32 upsum=True want_y=False",
    "pixelnorm_lrelu_bwd gp=[64,32,2,2] y=[64,32,2,2] rn=[64,1,2,2] from_p=True",
    "group_means scores=[64,1] groups=1",
]
CRITIC_SWEEP = [
    "conv3x3_wgrad x=[192,48,128,128] gy=[192,64,128,128] gw=[64,48,3,3] gb=[64] accumulate=False bias_n=128 defer='WgradDefer'",
    "conv3x3_wgrad x=[192,64,64,64] gy=[192,64,64,64] gw=[64,64,3,3] gb=[64] accumulate=False bias_n=128 defer='WgradDefer'",
    "conv3x3_wgrad x=[192,64,64,64] gy=[192,80,64,64] gw=[80,64,3,3] gb=[80] accumulate=False bias_n=128 defer='WgradDefer'",
    "conv3x3_wgrad x=[192,80,32,32] gy=[192,80,32,32] gw=[80,80,3,3] gb=[80] accumulate=False bias_n=128 defer='WgradDefer'",
    "conv3x3_wgrad x=[192,80,32,32] gy=[192,96,32,32] gw=[96,80,3,3] gb=[96] accumulate=False bias_n=128 defer='WgradDefer'",
    "conv3x3_wgrad x=[192,96,16,16] gy=[192,96,16,16] gw=[96,96,3,3] gb=[96] accumulate=False bias_n=128 defer='WgradDefer'",
    "conv3x3_wgrad x=[192,96,16,16] gy=[192,112,16,16] gw=[112,96,3,3] gb=[112] accumulate=False bias_n=128 defer='WgradDefer'",
    "conv3x3_wgrad x=[192,112,8,8] gy=[192,112,8,8] gw=[112,112,3,3] gb=[112] accumulate=False bias_n=128 defer='WgradDefer'",
    "conv3x3_wgrad x=[192,112,8,8] gy=[192,128,8,8] gw=[128,112,3,3] gb=[128] accumulate=False bias_n=128 defer='WgradDefer'",
    "conv3x3_wgrad x=[192,128,4,4] gy=[192,128,4,4] gw=[128,128,3,3] gb=[128] accumulate=False bias_n=128 defer='WgradDefer'",
    "conv3x3_wgrad x=[192,128,4,4] gy=[192,144,4,4] gw=[144,128,3,3] gb=[144] accumulate=False bias_n=128 defer='WgradDefer'",
    "conv3x3_wgrad x=[192,144,2,2] gy=[192,144,2,2] gw=[144,144,3,3] gb=[144] accumulate=False bias_n=128 defer='WgradDefer'",
    "conv3x3_wgrad x=[192,144,2,2] gy=[192,160,2,2] gw=[160,144,3,3] gb=[160] accumulate=False bias_n=128 defer='WgradDefer'",
    "conv3x3_wgrad x=[192,160,1,1] gy=[192,160,1,1] gw=[160,160,3,3] gb=[160] accumulate=False bias_n=128 defer='WgradDefer'",
]
GENERATOR_SWEEP = [
    "conv3x3_wgrad x=[64,64,64,64] gy=[64,48,128,128] gw=[48,64,3,3] gb=[48] ups=True accumulate=False defer='WgradDefer'",
    "conv3x3_wgrad x=[64,64,64,64] gy=[64,64,64,64] gw=[64,64,3,3] gb=[64] accumulate=False defer='WgradDefer'",
    "conv3x3_wgrad x=[64,80,32,32] gy=[64,64,64,64] gw=[64,80,3,3] gb=[64] ups=True accumulate=False defer='WgradDefer'",
    "conv3x3_wgrad x=[64,80,32,32] gy=[64,80,32,32] gw=[80,80,3,3] gb=[80] accumulate=False defer='WgradDefer'",
    "conv3x3_wgrad x=[64,96,16,16] gy=[64,80,32,32] gw=[80,96,3,3] gb=[80] ups=True accumulate=False defer='WgradDefer'",
    "conv3x3_wgrad x=[64,96,16,16] gy=[64,96,16,16] gw=[96,96,3,3] gb=[96] accumulate=False defer='WgradDefer'",
    "conv3x3_wgrad x=[64,112,8,8] gy=[64,96,16,16] gw=[96,112,3,3] gb=[96] ups=True accumulate=False defer='WgradDefer'",
    "conv3x3_wgrad x=[64,112,8,8] gy=[64,112,8,8] gw=[112,112,3,3] gb=[112] accumulate=False defer='WgradDefer'",
    "conv3x3_wgrad x=[64,128,4,4] gy=[64,112,8,8] gw=[112,128,3,3] gb=[112] ups=True accumulate=False defer='WgradDefer'",
    "conv3x3_wgrad x=[64,128,4,4] gy=[64,128,4,4] gw=[128,128,3,3] gb=[128] accumulate=False defer='WgradDefer'",
    "conv3x3_wgrad x=[64,32,2,2] gy=[64,128,4,4] gw=[128,32,3,3] gb=[128] ups=True accumulate=False defer='WgradDefer'",
    "conv3x3_wgrad x=[64,32,2,2] gy=[64,32,2,2] gw=[32,32,3,3] gb=[32] accumulate=False defer='WgradDefer'",
]


def test_headline_step_launches_are_all_covered(monkeypatch):
    """Every launch of the step is in LAUNCHES (a SUBSET: any new shape or flag combination fails until it is added and checked
    below), and the two weight-gradient sweeps are the committed ones, layer for layer."""
    c = step_census(monkeypatch, LEVEL, BATCH)
    got = [spec(r) for r in c.distinct if _launch(r[0])]
    missing = [s for s in got if s not in set(LAUNCHES)]
    assert not missing, "launches of the level-5 batch-64 step without a headline-shape check:\n" + "\n".join(missing)
    assert all(r[0] != "conv3x3_wgrad" or dict(r[1]).get("defer") == "WgradDefer" for r in c.calls)
    assert sweeps_of(c.calls) == [CRITIC_SWEEP, GENERATOR_SWEEP]


@pytest.mark.parametrize("line", LAUNCHES, ids=[f"{i:03d}-{line.split()[0]}" for i, line in enumerate(LAUNCHES)])
def test_launch_against_float64(line):
    check_launch(line)


@pytest.mark.parametrize("sweep", ["critic", "generator"])
def test_weight_gradient_sweep(sweep):
    """One replay of the step's deferred weight-gradient sweep: the same layers, shapes and order into one WgradDefer, one flush
    (the grouped matrix launches and the one-launch slab reduction), every weight and bias gradient against float64 autograd of
    F.conv2d (through F.interpolate for the up-sampled inputs) in full."""
    check_sweep(CRITIC_SWEEP if sweep == "critic" else GENERATOR_SWEEP, sweep)
