"""bench.py --dump-outputs: the arrays of the last timed step as float32 / float64 .npy files,
the same from run to run, within the size bound; --steps sets the timed steps and the plain
line carries the headline keys without the --full measurements."""
import json
import os

import numpy as np
import pytest
import torch

import bench
from grok_amd.synth import synth_image


def test_sample_is_fixed_and_ordered():
    t = torch.arange(100000, dtype=torch.int32)
    whole = bench.sample(t.reshape(100, 1000), 100000, 1)
    assert whole.dtype == np.float32 and np.array_equal(whole, np.arange(100000, dtype=np.float32))
    a, b = bench.sample(t, 1000, 1), bench.sample(t.clone(), 1000, 1)
    assert a.shape == (1000,) and np.array_equal(a, b) and (np.diff(a) >= 0).all()
    assert not np.array_equal(a, bench.sample(t, 1000, 2))
    # the headline pair's four sampled arrays and three summaries stay under 64 MB
    assert 4 * (bench.DUMP_BUDGET // 4 // 4) * 4 + 3 * 3 * 8 + 7 * 128 <= 64 << 20


def test_threaded_synth_is_the_seeded_image():
    # three row chunks, the last one short
    assert np.array_equal(bench.synth_image_threads(2500, 48, 3, 12, 11), synth_image(2500, 48, 3, 12, 11))


@pytest.mark.gpu
def test_dump_outputs_of_a_plain_run(tmp_path, capsys):
    size, lines = 320, []
    for d in ("a", "b"):
        bench.main(["--gpus", "1", "--steps", "2", "--warmup", "1", "--size", str(size),
                    "--dump-outputs", str(tmp_path / d)])
        out = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
        assert len(out) == 1
        lines.append(json.loads(out[0]))
    res = lines[0]
    assert res["steps"] == 2 and res["warmup"] == 1 and res["ms_per_step"] > 0 and res["value"] > 0
    assert res["metric"] == bench.METRIC and res["unit"] == "Mpixels/s" and res["higher_is_better"] is True
    assert res["dtype"] == "int32 (5/3) + f32 (9/7)"
    assert not {"aux", "cpu_baseline", "per_config", "issue_roofline"} & set(res)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted("%s_%s.npy" % (c, k) for c in ("C2", "C3") for k in ("codestream", "decoded", "summary"))
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), n
        total += os.path.getsize(tmp_path / "a" / n)
    assert total <= 64 << 20
    # C2 is lossless: the decoded output is the seeded source image, and the summary describes the arrays
    img = synth_image(size, size, 3, 8, 10)
    dec, cs, summ = (np.load(tmp_path / "a" / ("C2_%s.npy" % k)) for k in ("decoded", "codestream", "summary"))
    assert np.array_equal(dec, img.reshape(-1).astype(np.float32))
    assert summ[0] == cs.size == res["config"]["codestream_bytes"] - np.load(tmp_path / "a" / "C3_summary.npy")[0]
    assert summ[1] == cs.astype(np.float64).sum() and summ[2] == img.astype(np.float64).sum()
    assert cs[0] == 0xFF and cs[1] == 0x4F   # SOC
