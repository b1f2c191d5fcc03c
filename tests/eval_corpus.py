"""The tiny corpus and checkpoint the `evaluate` tests run on: a few wav files of noise packed by create_dataset, and a freshly
initialised generator saved at a low level.  Needs the GPU (create_dataset runs on it)."""
import torch


def tiny_corpus(tmp_path, files: int, seed: int, level: int = 2, rand_channels: int = 8):
    """`files` stereo wav files of 256 * 1030 uniform samples drawn from a CPU generator seeded with `seed`, packed into
    `tmp_path / "data"` (two dataset entries per file), and the state of Generator(rand_channels, end_layer=level) built after
    torch.manual_seed(0), saved as `tmp_path / "gen{level}.pt"`.  Returns (data_dir, checkpoint) as strings."""
    import musicgan_amd
    from musicgan_amd.audio import wavio
    from musicgan_amd.networks import Generator
    rng = torch.Generator().manual_seed(seed)
    wav_dir, data_dir = tmp_path / "wav", tmp_path / "data"
    wav_dir.mkdir()
    for i in range(files):
        wavio.save(str(wav_dir / f"s{i}.wav"), torch.rand(2, 256 * 1030, generator=rng) - 0.5, 44100)
    musicgan_amd.create_dataset(str(wav_dir / "*.wav"), str(data_dir))
    torch.manual_seed(0)
    ck = str(tmp_path / f"gen{level}.pt")
    torch.save(Generator(rand_channels, end_layer=level).state_dict(), ck)
    return str(data_dir), ck
