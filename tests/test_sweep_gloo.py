"""--taps over N ranks on the host: the triplet shard and one pair of score gathers per tap over gloo (--selftest_shard: a
stand-in scorer, no GPU) must print, tap for tap, what the one-rank run prints."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env():
    return {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT",
                                                            "LOCAL_WORLD_SIZE")}


def _tree(root):
    from PIL import Image
    for c in range(2):
        for i in range(3):
            for l in range(2):
                d = os.path.join(root, f"cls{c}", f"inst{i}", f"light{l}")
                os.makedirs(d)
                for k in range(3):
                    Image.new("RGB", (8, 8), (c * 40, i * 40, k * 40)).save(os.path.join(d, f"im{k}.png"))


def test_taps_sharded_over_two_ranks_match_one_rank(tmp_path):
    _tree(str(tmp_path))
    base = [sys.executable, "-m", "diffsim_amd", "--image_path", str(tmp_path), "--target_step", "600", "--similarity", "cosine",
            "--seed", "2334", "--selftest_shard", "--taps", "up_blocks:1", "down_blocks:0", "mid_blocks:0", "up_blocks:2"]
    r1 = subprocess.run(base, capture_output=True, text=True, env=_env(), cwd=ROOT, timeout=300)
    assert r1.returncode == 0, r1.stderr[-2000:]
    r2 = subprocess.run(base + ["--ngpu", "2"], capture_output=True, text=True, env=_env(), cwd=ROOT, timeout=600)
    assert r2.returncode == 0, r2.stderr[-2000:]
    keep = lambda out: [ln for ln in out.splitlines() if not ln.startswith("[Gloo]")]      # (gloo's own connection notes)
    lines = keep(r1.stdout)
    assert lines == keep(r2.stdout) and lines[0] == "=========seed 2334========="
    heads = [ln for ln in lines if ln.startswith("Experiment on")]
    assert heads == [f"Experiment on {b}, layer [{l}], timestep 600:" for b, l in
                     (("up_blocks", 1), ("down_blocks", 0), ("mid_blocks", 0), ("up_blocks", 2))]
    acc = [ln for ln in lines if ln.startswith("Accuracy")]
    assert len(acc) == 4 and len(set(acc)) > 1            # each tap its own gathered scores
