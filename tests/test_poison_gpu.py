"""Every op on poisoned memory with guard bands (tests/poison.py).

Rule R, for every case: the case runs under fill 0x00 and again under fill 0xFF with the same seeded finite inputs (the zero pass
first); no guard band is damaged in either run, no argument that `poison.INPLACE` does not declare has changed, the digests of the
two runs are equal entry by entry, and no floating output of the 0xFF run holds a NaN or an infinity (integer and byte outputs
are exempt from that point only).  A case is the body of an existing test -- called with its own committed parameters, so its
float64 comparison also judges both poisoned runs -- or a whole update of `ProGANStepper`.

(a) every line of the headline census and its two deferred sweeps; (b) the per-op parity tests over their committed shape lists;
(c) one critic and one generator update with the real FusedAdam step at every level; (d) the audio and metric ops; (e) nothing
left out: `REACHES` names, per group of cases, the ops it must reach (checked against the census of each case as it runs), and
`test_every_op_has_a_poison_case` checks that every public function of `ops` and the library calls of `optim` and `create_dataset`
are reached or excluded with a reason; the six side modules carry their own poisoned cases (see `LIBRARY_CALLS_OUTSIDE_OPS`)."""
import contextlib
import importlib
import itertools
import random
import shutil

import numpy as np
import pytest
import torch

import poison
import test_headline_shapes_gpu as H
from routing_census import parse, public_functions

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# determinism exemption of point 3: ops of which two 0x00 runs were SEEN to differ (test_exempt_ops_are_really_not_deterministic)
NOT_BITWISE = ()


@contextlib.contextmanager
def library_calls():
    """the names of the C entry points called through `_lib.check` (ops, its six side modules, optim, create_dataset), as a set"""
    from musicgan_amd import _lib, avg_ops, gl_ops, loud_ops, nn_ops, ops, optim, pv_ops, ssim_ops
    seen = set()
    real = _lib.check

    def check(rc, what):
        seen.add(what)
        return real(rc, what)
    with pytest.MonkeyPatch.context() as mp:
        for m in (_lib, ops, optim, ssim_ops, avg_ops, nn_ops, gl_ops, pv_ops, loud_ops):
            mp.setattr(m, "check", check)
        yield seen


def _seed():
    torch.manual_seed(1234)
    np.random.seed(1234)
    random.seed(1234)


REACHED = {}   # group -> ops reached by every case of it that ran (for the report at the end of the session's output)


def run_case(group, body, *, digest="clone", fixtures=()):
    """R over `body(**fixtures)`; the fixtures are made anew inside each poisoned run (a MonkeyPatch that is undone before the ops
    are unwrapped, a directory per fill)."""
    def case(p):
        _seed()
        with pytest.MonkeyPatch.context() as mp, library_calls() as lib:
            kw = {}
            for name, value in fixtures:
                if name == "monkeypatch":
                    kw[name] = mp
                elif name == "tmp_path":   # the same directory for both fills: file names are part of the recorded calls
                    kw[name] = value / "case"
                    shutil.rmtree(kw[name], ignore_errors=True)
                    kw[name].mkdir()
                else:
                    kw[name] = value
            try:
                body(**kw)
            except pytest.skip.Exception as e:   # the existing test declines this parameter set: nothing to judge
                p.declined = str(e)
            torch.cuda.synchronize()
        p.lib = set(lib)
    a, b = poison.rule(case, digest=digest, exempt=NOT_BITWISE)
    if getattr(a, "declined", None) or getattr(b, "declined", None):
        print(f"POISON {group}: declined by the test itself ({a.declined})")
        return a, b
    for p in (a, b):
        reached = p.census.ops() | p.lib
        missing = set(REACHES.get(group, ())) - reached
        assert not missing, f"{group}: the registry says it reaches {sorted(missing)}, the census of this case does not"
        REACHED[group] = REACHED.get(group, reached) & reached
    print(f"POISON {group}: {len(b.calls)} calls ({b.launches} with nested), ops {sorted(b.census.ops() | b.lib)}")
    return a, b


def _param_sets(fn):
    """the keyword sets of a test function's own parametrize marks (their product)"""
    axes = []
    for m in getattr(fn, "pytestmark", []):
        if m.name == "parametrize":
            names = [n.strip() for n in m.args[0].split(",")] if isinstance(m.args[0], str) else list(m.args[0])
            axes.append([dict(zip(names, v if len(names) > 1 else (v,))) for v in m.args[1]])
    out = []
    for combo in itertools.product(*axes):
        kw = {}
        for d in combo:
            kw.update(d)
        out.append(kw)
    return out


def _fixtures_of(fn):
    import inspect
    return [n for n in inspect.signature(fn).parameters if n in ("monkeypatch", "tmp_path", "capsys")]


def _cases(table):
    out = []
    for module, names in table:
        mod = importlib.import_module(module)
        for name in names:
            keep = None
            if isinstance(name, tuple):
                name, keep = name
            fn = getattr(mod, name)
            for i, kw in enumerate(_param_sets(fn)):
                if keep is None or keep(kw):
                    out.append(pytest.param(module, name, kw, id=f"{module[5:-4]}.{name[5:]}-{i}"))
    return out


def _run_existing(module, name, kw, tmp_path, capsys):
    fn = getattr(importlib.import_module(module), name)
    fx = [(n, {"tmp_path": tmp_path, "capsys": capsys}.get(n)) for n in _fixtures_of(fn)]
    return run_case(f"{module}.{name}", lambda **f: fn(**kw, **f), fixtures=fx)


# ------------------------------------------------------------------ (a) the headline launches
@pytest.mark.parametrize("line", H.LAUNCHES, ids=[f"{i:03d}-{line.split()[0]}" for i, line in enumerate(H.LAUNCHES)])
def test_headline_launch(line):
    a, b = run_case("headline", lambda: H.test_launch_against_float64(line))
    assert parse(line)[0] in b.census.ops()


@pytest.mark.parametrize("sweep", ["critic", "generator"])
def test_headline_weight_gradient_sweep(sweep):
    a, b = run_case("headline sweep", lambda: H.test_weight_gradient_sweep(sweep))
    flushes = [c for c in b.calls if c[0] == "WgradDefer.flush"]
    lines = H.CRITIC_SWEEP if sweep == "critic" else H.GENERATOR_SWEEP
    assert len(flushes) == 1 and len(flushes[0][2]) == 2 * len(lines)   # gw and gb of every layer, digested at the one flush


def test_a_flipped_bit_is_reported_with_its_launch():
    """R bites on the device: one bit of one output of one headline launch, changed in the 0xFF run only"""
    line = H.LAUNCHES[3]
    assert line.startswith("pixelnorm_fwd")

    def flip(name, rec, result):
        if name == "pixelnorm_fwd":
            result[0].view(torch.int32).reshape(-1)[5] ^= 1
        return result

    runs = []
    for fill in (0x00, 0xFF):
        with poison.poisoned(fill) as p:
            p.post = flip if fill == 0xFF else None
            _seed()
            try:
                H.test_launch_against_float64(line)
            except AssertionError:   # one ulp may or may not cross the float64 bound
                pass
        runs.append(p)
    with pytest.raises(poison.PoisonError) as e:
        poison.compare(*runs)
    msg = str(e.value)
    assert msg.startswith("pixelnorm_fwd: output return[0] of call 0") and "bytes +20 .. +20 of it (1 bytes)" in msg
    assert "call: pixelnorm_fwd y=[64,128,4,4]" in msg


# ------------------------------------------------------------------ (b) the per-op parity tests over their committed shape lists
PARITY = [
    ("test_ops_gpu", ["test_conv3x3_fwd_bias_lrelu", "test_conv3x3_dgrad_and_mask", "test_conv3x3_ups_pixnorm", "test_conv3x3_wgrad",
                      "test_conv3x3_wgrad_upsampled_input", "test_conv1x1_all_modes", "test_elementwise_ops",
                      "test_linear_and_gp_helpers", "test_conv3x3_fused_avgpool_output",
                      "test_upconv3x3_subpixel_matches_upsample_conv", "test_upconv3x3_dgrad_matches_autograd",
                      "test_wino3x3_fwd_dgrad_mask_pool", "test_conv1x1_wgrad_bias_n",
                      "test_wino3x3_fade_in_epilogues_equal_the_separate_kernels", "test_wino3x3_pixnorm",
                      "test_wino_wgrad_matches_autograd", "test_wino_wgrad_scalar_addressed_loads_equal_the_general_form",
                      "test_blend_lrelu_bwd_equals_the_four_kernels_it_replaces",
                      "test_pixelnorm_bwd_lds_path_is_bitwise_the_two_pass_kernel", "test_pixelnorm_bwd_small_maps",
                      "test_pack_multi_equals_single_tensor_packs", "test_conv3x3_split_k_small_maps",
                      "test_pixelnorm_fwd_small_maps", "test_conv1x1_few_out_split_channels",
                      "test_group_means_and_deferred_wgrad_reduce", "test_grouped_wgrad_launch", "test_conv3x3_wgrad_on_1x1_maps"]),
    ("test_winoups_gpu", ["test_forward_matches_fp64_and_the_subpixel_kernel", "test_data_gradient_matches_autograd",
                          "test_forward_with_the_head_in_the_epilogue"]),
    ("test_wino_strip_gpu", ["test_strip_kernel_equals_the_staged_kernel_bit_for_bit",
                             "test_strip_kernel_against_fp64_at_level_6_7_shapes"]),
    ("test_wgrad_rows_gpu", ["test_rows_kernel_matches_autograd_and_the_chunk_kernels", "test_rows_kernel_with_upsampled_input",
                             "test_rows_kernel_inside_a_deferred_sweep"]),
    ("test_fade_ends_gpu", ["test_stem_pair_forward_and_tangent", "test_stem_pair_gx", "test_head_pair_and_blend_backward",
                            "test_conv1x1_accumulate", "test_conv1x1_wgrad_single_launch", "test_gp_apply_equals_finish_and_scale",
                            "test_gen_head_bwd_matches_the_three_launches_and_autograd"]),
    ("test_smallnet_gpu", ["test_conv_chain_with_pool_and_linear", "test_generator_head_forward_and_backward",
                           "test_critic_tail_data_gradient_and_tangent", "test_full_width_layers_and_8x8_maps",
                           "test_conv3x3_small_every_epilogue", "test_conv3x3_small_with_pixelnorm_folded_into_its_staging"]),
]


@pytest.mark.parametrize("module, name, kw", _cases(PARITY))
def test_parity_body(module, name, kw, tmp_path, capsys):
    _run_existing(module, name, kw, tmp_path, capsys)
    if name == "test_conv1x1_wgrad_single_launch":
        # the ticket counters of the single-launch form live in a device symbol, not in a workspace: the kernel must leave them at
        # zero, so the same case passes a second time in this process
        _run_existing(module, name, kw, tmp_path, capsys)


@pytest.mark.parametrize("shape", [(3, 37, 5, 7), (2, 160, 2, 2), (2, 48, 32, 32)])
def test_pixelnorm_bwd_alone(shape):
    """`ops.pixelnorm_bwd` (the PixelNorm backward without the LeakyReLU mask) has no parity test of its own to re-run: float64
    autograd of y / sqrt(mean_c y^2 + 1e-8), at 3e-6 of the largest element -- the bound the headline checks give the same kernel."""
    from musicgan_amd import ops

    def body():
        g = torch.Generator(device=DEV).manual_seed(5)
        y, gp = torch.randn(shape, device=DEV, generator=g), torch.randn(shape, device=DEV, generator=g)
        _, rn = ops.pixelnorm_fwd(y)
        got = ops.pixelnorm_bwd(gp, y, rn)
        y64 = y.double().cpu().requires_grad_(True)
        (H._pn(y64)[0] * gp.double().cpu()).sum().backward()
        err = float((got.double().cpu() - y64.grad).abs().max())
        assert err <= 3e-6 * float(y64.grad.abs().max()), err

    run_case("pixelnorm_bwd", body)


# ------------------------------------------------------------------ (c) whole updates at every level
STEPS = [(3, 8, 0.5), (4, 8, 0.5), (5, 6, 0.5), (5, 6, 1.0), (5, 6, 0.0), (6, 2, 0.5), (7, 1, 0.5),
         (0, 6, 0.5), (1, 6, 0.5), (2, 6, 0.5), (2, 64, 0.5)]  # level 0 has no fade-in: alpha is unused there


@pytest.mark.parametrize("level, batch, alpha", STEPS)
def test_whole_update(level, batch, alpha):
    """One critic and one generator update (eager, the real FusedAdam step: its launch and the packing it triggers are inside the
    poisoned region, the nets and the moments are guarded allocations); R over every launch and over the final weights and moments."""
    import bench
    from musicgan_amd.optim import FusedAdam
    from musicgan_amd.train_step import ProGANStepper
    final = {}

    def body(monkeypatch):
        monkeypatch.setenv("MG_GRAPHS", "0")
        gen, disc = bench.build_nets(level, 32, DEV)
        og = FusedAdam(gen.parameters(), lr=1e-3, betas=(0.0, 0.9))
        od = FusedAdam(disc.parameters(), lr=1e-3, betas=(0.0, 0.9))
        st = ProGANStepper(gen, disc, og, od, 32)
        side = 4 << level  # bench.LEVEL_SIDE where that has the level (test_launch_checks_cpu.py); levels 0-2 are below its table
        rng = torch.Generator(device=DEV).manual_seed(1234)
        x_real = torch.rand(batch, 2, side, side, device=DEV, generator=rng) * 2 - 1
        z = torch.randn(batch, 32, 2, 2, device=DEV, generator=rng)
        eps = torch.rand(batch, 1, 1, 1, device=DEV, generator=rng)
        st.d_step(x_real, alpha, z=z, eps=eps)
        st.g_step(batch, alpha, DEV, z=z)
        torch.cuda.synchronize()
        out = []
        for net, opt in ((gen, og), (disc, od)):
            for p in net.parameters():
                s = opt.state.get(p, {})
                for what, t in (("w", p), ("m", s.get("exp_avg")), ("v", s.get("exp_avg_sq")), ("t", s.get("step_dev"))):
                    if t is not None:
                        assert bool(torch.isfinite(t.detach().float()).all()), f"non-finite {what} after the update"
                        out.append(poison.hash_bits(t.detach()))
        final.setdefault("runs", []).append(out)

    a, b = run_case("whole update", body, digest="hash", fixtures=[("monkeypatch", None)])
    r0, r1 = final["runs"]
    assert len(r0) == len(r1) and len(r0) > 0
    assert r0 == r1, "the final weights / Adam moments differ between fill 0x00 and fill 0xFF"
    assert "mg_adam_step_dev" in b.lib


# ------------------------------------------------------------------ (d) the audio and metric ops
AUDIO = [
    ("test_audio_gpu", ["test_wav_to_stft_and_codec_match_reference_golden", "test_inverse_codec_matches_reference_golden",
                        "test_stft_from_pcm_frames_equals_the_normalised_mono_path", "test_codec_odd_sizes_against_oracle",
                        "test_device_crc32_of_the_float64_payload_equals_zlib", "test_stft_with_other_window_and_hop_sizes"]),
    ("test_ops_gpu", ["test_stft_kernel_matches_oracle_and_torch", "test_input_transform_matches_the_tensor_expressions"]),
    ("test_resample_gpu", [("test_resample_matches_float64_torchaudio_form", lambda kw: (kw["orig"], kw["new"]) in
                            ((48000, 44100), (192000, 44100), (44100, 48000))),
                           "test_resample_of_strided_rows_and_leading_dims", "test_fused_pcm_path_is_bit_identical_to_the_composition"]),
    ("test_flac_gpu", [("test_round_trip_matrix", lambda kw: kw["seed"] < 4)]),
    ("test_flac_encode_gpu", [("test_round_trip", lambda kw: kw["ch"] in (1, 2) and kw["kind"] in ("music", "noise")),
                              "test_encoding_is_deterministic_and_takes_any_layout"]),
    ("test_vorbis_gpu", ["test_fixture_matches_the_reader_and_is_deterministic"]),
    ("test_vorbis_streams_gpu", [("test_random_streams_match_the_reader", lambda kw: kw["case"] in (2, 5))]),
    ("test_vorbis_encode_gpu", [("test_round_trip_frame_count", lambda kw: kw["ch"] in (1, 2) and kw["rate"] == 44100 and
                                 kw["n"] in (1025, 3 * 44100)), "test_deterministic_and_layouts"]),
    ("test_swd_gpu", [("test_pyramid_matches_the_float64_definition", lambda kw: kw["kind"] == "random"),
                      "test_gather_copies_patches_and_sums_in_float64",
                      ("test_projection_within_the_dot_product_bound", lambda kw: kw["m"] in (63, 1000) and kw["d"] == 128),
                      ("test_segmented_sort_equals_torch_sort", lambda kw: kw["s"] == 3 and kw["m"] in (1, 65, 4095, 40961)),
                      "test_swd_end_to_end_matches_the_float64_definition_bit_stable_over_batching",
                      "test_sliced_wasserstein_one_repeat_is_symmetric_and_matches"]),
]


@pytest.mark.parametrize("module, name, kw", _cases(AUDIO))
def test_audio_and_metric_body(module, name, kw, tmp_path, capsys):
    _run_existing(module, name, kw, tmp_path, capsys)


def test_vorbis_encoder_output_words_are_zeroed_by_its_own_kernel():
    """`vorbis_encode_prepare` hands the encoder an `empty` output buffer and the packing kernel ORs bits into its words: under
    0xFF poison the stream is the one of the 0x00 run and decodes with the test reader only if a kernel of the encoder zeroes the
    words first.  The digest of an encoder is its byte stream."""
    import vorbis_reader as R
    from musicgan_amd import ops
    streams = {}

    def body():
        g = torch.Generator().manual_seed(7)
        for ch in (1, 2):
            x = (torch.rand(ch, 5000, generator=g) - 0.5) * 0.8
            streams.setdefault(ch, []).append(bytes(ops.vorbis_encode(x, 44100, 3.0).numpy().tobytes()))

    run_case("vorbis encoder zeroing", body)
    for ch, (s0, s1) in streams.items():
        assert s0 == s1, f"{ch}-channel Ogg stream differs between the fills"
        assert R.decode_file(s1).shape == (5000, ch)


def test_create_dataset_one_file(tmp_path):
    """`create_dataset` of one WAV file with one loader thread (the calls of the main thread then come in a fixed order): the stacked
    codec output and the library call that writes the samples (`mg_pt_write_samples`, called outside `ops`); the digest is the
    bytes of the files written."""
    import glob
    import musicgan_amd
    from musicgan_amd import audio
    from musicgan_amd.audio import wavio
    files = []

    def body(tmp_path, monkeypatch):
        monkeypatch.setenv("MG_LOADER_THREADS", "1")
        monkeypatch.delenv("RANK", raising=False)
        monkeypatch.delenv("WORLD_SIZE", raising=False)
        (tmp_path / "in").mkdir()
        g = torch.Generator().manual_seed(11)
        wavio.save(str(tmp_path / "in" / "a.wav"), (torch.rand(2, 256 * 700 + 91, generator=g) - 0.5) * 0.9, 44100)
        musicgan_amd.create_dataset(str(tmp_path / "in" / "*.wav"), str(tmp_path / "out"))
        ds = audio.AudioDataset(str(tmp_path / "out"))
        assert len(ds) >= 1 and all(bool(torch.isfinite(ds[i]).all()) for i in range(len(ds)))
        files.append({p.rsplit("/", 1)[1]: open(p, "rb").read() for p in sorted(glob.glob(str(tmp_path / "out" / "*")))})

    run_case("create_dataset", body, fixtures=[("tmp_path", tmp_path), ("monkeypatch", None)])
    assert files[0] == files[1] and len(files[0]) >= 1


# ------------------------------------------------------------------ (e) nothing left out
# group of cases -> the ops every case of the group reaches (checked by run_case against the census of each case)
REACHES = {
    "headline sweep": ("conv3x3_wgrad", "WgradDefer.flush"),
    "whole update": ("conv3x3", "conv3x3_wgrad", "WgradDefer.flush", "pack_multi", "group_means", "gp_interp", "linear1_fwd",
                     "linear1_bwd", "mg_adam_step_dev"),
    "pixelnorm_bwd": ("pixelnorm_bwd", "pixelnorm_lrelu_bwd"),
    "vorbis encoder zeroing": ("vorbis_encode", "vorbis_encode_prepare", "vorbis_encode_run"),
    "test_ops_gpu.test_conv3x3_fwd_bias_lrelu": ("conv3x3", "pack_conv3x3"),
    "test_ops_gpu.test_conv3x3_wgrad": ("conv3x3_wgrad",),
    "test_ops_gpu.test_conv1x1_all_modes": ("conv1x1", "conv1x1_wgrad", "workspace"),
    "test_ops_gpu.test_elementwise_ops": ("pixelnorm_fwd", "channel_sum", "pixelnorm_lrelu_bwd", "upsample2x_fwd", "upsample2x_bwd",
                                          "avgpool2_fwd", "avgpool2_bwd", "lrelu_bwd", "axpby", "blend_up"),
    "test_ops_gpu.test_linear_and_gp_helpers": ("linear1_fwd", "linear1_bwd", "gp_interp", "sumsq_per_sample", "scale_per_sample",
                                                "gp_finish"),
    "test_ops_gpu.test_upconv3x3_subpixel_matches_upsample_conv": ("upconv3x3", "pack_upconv3x3"),
    "test_ops_gpu.test_upconv3x3_dgrad_matches_autograd": ("upconv3x3_dgrad", "pack_upconv3x3_dgrad"),
    "test_ops_gpu.test_wino3x3_fwd_dgrad_mask_pool": ("conv3x3", "pack_wino3x3"),
    "test_ops_gpu.test_wino3x3_fade_in_epilogues_equal_the_separate_kernels": ("conv3x3_fade",),
    "test_ops_gpu.test_blend_lrelu_bwd_equals_the_four_kernels_it_replaces": ("blend_lrelu_bwd",),
    "test_ops_gpu.test_pack_multi_equals_single_tensor_packs": ("pack_multi",),
    "test_ops_gpu.test_group_means_and_deferred_wgrad_reduce": ("group_means", "WgradDefer.flush"),
    "test_winoups_gpu.test_forward_matches_fp64_and_the_subpixel_kernel": ("winoups3x3", "pack_winoups3x3"),
    "test_winoups_gpu.test_data_gradient_matches_autograd": ("winoups3x3_dgrad",),
    "test_winoups_gpu.test_forward_with_the_head_in_the_epilogue": ("winoups3x3_head",),
    "test_fade_ends_gpu.test_stem_pair_forward_and_tangent": ("stem_pair",),
    "test_fade_ends_gpu.test_stem_pair_gx": ("stem_pair_gx",),
    "test_fade_ends_gpu.test_head_pair_and_blend_backward": ("head_pair", "blend_up_bwd"),
    "test_fade_ends_gpu.test_gp_apply_equals_finish_and_scale": ("gp_apply",),
    "test_fade_ends_gpu.test_gen_head_bwd_matches_the_three_launches_and_autograd": ("gen_head_bwd",),
    "test_smallnet_gpu.test_conv_chain_with_pool_and_linear": ("SmallNet.run", "pack_smallnet"),
    "test_smallnet_gpu.test_conv3x3_small_every_epilogue": ("conv3x3_small",),
    "test_smallnet_gpu.test_conv3x3_small_with_pixelnorm_folded_into_its_staging": ("conv3x3_small_pn",),
    "test_audio_gpu.test_wav_to_stft_and_codec_match_reference_golden": ("codec_fwd",),
    "test_audio_gpu.test_inverse_codec_matches_reference_golden": ("codec_inv",),
    "test_audio_gpu.test_stft_from_pcm_frames_equals_the_normalised_mono_path": ("stft_1024_pcm", "stft_1024"),
    "test_audio_gpu.test_device_crc32_of_the_float64_payload_equals_zlib": ("crc32_of_float64",),
    "test_audio_gpu.test_stft_with_other_window_and_hop_sizes": ("stft_generic",),
    "test_ops_gpu.test_input_transform_matches_the_tensor_expressions": ("input_transform",),
    "test_resample_gpu.test_resample_matches_float64_torchaudio_form": ("resample_rows", "resample_bank"),
    "test_resample_gpu.test_fused_pcm_path_is_bit_identical_to_the_composition": ("resample_pcm", "pcm_to_mono"),
    "test_flac_gpu.test_round_trip_matrix": ("flac_decode",),
    "create_dataset": ("stft_1024_pcm", "codec_fwd", "mg_pt_write_samples"),
    "test_flac_encode_gpu.test_round_trip": ("flac_encode",),
    "test_vorbis_gpu.test_fixture_matches_the_reader_and_is_deterministic": ("vorbis_decode", "vorbis_prepare", "vorbis_run"),
    "test_swd_gpu.test_pyramid_matches_the_float64_definition": ("swd_pyr_down", "swd_pyr_lap"),
    "test_swd_gpu.test_gather_copies_patches_and_sums_in_float64": ("swd_gather",),
    "test_swd_gpu.test_projection_within_the_dot_product_bound": ("swd_project",),
    "test_swd_gpu.test_segmented_sort_equals_torch_sort": ("swd_sort_segments_",),
    "test_swd_gpu.test_swd_end_to_end_matches_the_float64_definition_bit_stable_over_batching": ("swd_stats_finish", "swd_distance"),
}

# functions that launch nothing and allocate nothing on the device
EXCLUDED = {
    "packed_floats": "host query of a packed layout's size",
    "wino_wgrad_form": "host query of the weight-gradient form",
    "wgrad_group_chunks": "reads an environment variable",
    "fuse_ends": "reads an environment variable",
    "resample_len": "host arithmetic",
    "resample_bank_host": "builds the bank in host memory",
    "flac_padded_bytes": "host arithmetic",
    "flac_streaminfo": "formats the STREAMINFO block on the host",
    "flac_encode_args": "argument checks on the host",
    "vorbis_encode_args": "argument checks on the host",
}
# the library calls made outside `ops` that the cases of this file must reach: optim.py and create_dataset.py.  The side modules
# (ssim_ops, avg_ops, nn_ops, gl_ops, pv_ops, loud_ops) call the library too; each has its `*_on_poisoned_memory` test next to its
# parity tests (test_msssim_gpu, test_ema_gpu, test_nn_gpu, test_griffinlim_gpu, test_phasevocoder_gpu, test_loudness_gpu), and
# `library_calls` sees their calls wherever a case of this file reaches one.
LIBRARY_CALLS_OUTSIDE_OPS = ("mg_adam_step_dev", "mg_pt_write_samples")


def test_every_op_has_a_poison_case():
    from musicgan_amd import ops
    from routing_census import LAUNCHES_OF_CLASSES
    names = [n for n, _ in public_functions(ops)] + [f"{c}.{m}" for c, m in LAUNCHES_OF_CLASSES] + list(LIBRARY_CALLS_OUTSIDE_OPS)
    covered = {op for group in REACHES.values() for op in group} | {parse(line)[0] for line in H.LAUNCHES}
    for n in EXCLUDED:
        assert n in names and n not in covered, f"EXCLUDED names {n}, which is not a function of ops or has a case"
    missing = [n for n in names if n not in covered and n not in EXCLUDED and not n.endswith("_supported")]
    assert not missing, f"ops without a poison case: {missing}"
    groups = {f"{m}.{n if isinstance(n, str) else n[0]}" for m, ns in PARITY + AUDIO for n in ns} | \
        {"headline sweep", "whole update", "vorbis encoder zeroing", "pixelnorm_bwd", "create_dataset"}
    assert set(REACHES) <= groups, f"REACHES names groups that do not run: {sorted(set(REACHES) - groups)}"


def test_exempt_ops_are_really_not_deterministic():
    """the determinism exemption is empty; an entry would have to be shown here by two 0x00 runs that differ"""
    assert NOT_BITWISE == ()
