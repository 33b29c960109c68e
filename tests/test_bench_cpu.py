"""bench.py's launch contract on CPU: the single-process run, the
driver's multi-rank form (``torch.distributed.run --nproc-per-node N``: one DP
replica per rank, barriers + max-over-ranks timing, summed tokens) and ``--tp``
(one model sharded over the ranks: rank 0 engine + HTTP stack, ranks > 0 in the TP
worker loop), over gloo with a tiny random-init Llama. The GPU form is the same
code with RCCL; the driver runs it on MI355X."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--device", "cpu", "--model", "tiny-llama", "--concurrency", "2", "--input-len", "16",
        "--output-len", "4", "--steps", "1", "--warmup", "1", "--num-kv-blocks", "256"]


def _run(cmd):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2")
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]  # rank 0 prints exactly one line
    return lines[0]


def _torchrun(n, port, extra):
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
            "--master-addr", "127.0.0.1", f"--master-port={port}", "bench.py", "--gpus", str(n)] + extra


def test_bench_single_process_gateway():
    out = _run([sys.executable, "bench.py"] + ARGS)
    assert out["n_gpus"] == 1 and out["config"]["parallelism"] == "tp1" and out["path"] == "gateway"
    assert out["value"] > 0 and out["p50_ttft_ms"] > 0 and out["steps"] == 1 and out["warmup"] == 1
    assert abs(out["value"] - 2 * 4 / (out["ms_per_step"] / 1000)) / out["value"] < 0.01


@pytest.mark.parametrize("tp", [1, 2])
def test_bench_two_ranks(tp):
    out = _run(_torchrun(2, 29650 + tp, ARGS + ["--tp", str(tp)]))
    assert out["n_gpus"] == 2
    if tp == 1:  # weak scaling: two replicas, tokens summed over ranks
        assert out["config"]["parallelism"] == "dp2" and out["scaling"] == "weak"
        assert out["config"]["global_batch"] == 4
        tokens = 2 * 2 * 4
    else:  # one replica sharded over both ranks
        assert out["config"]["parallelism"] == "tp2" and out["scaling"] == "strong"
        assert out["config"]["tp"] == 2 and out["config"]["global_batch"] == 2
        tokens = 2 * 4
    assert abs(out["value"] - tokens / (out["ms_per_step"] / 1000)) / out["value"] < 0.01


def test_free_port_disjoint_per_local_rank(monkeypatch):
    """DP replicas under torchrun draw gateway/router/engine ports from disjoint
    per-LOCAL_RANK ranges, distinct within a process."""
    from hipserve.bench import local_stack

    got = {}
    for r in range(8):
        monkeypatch.setenv("WORLD_SIZE", "8")
        monkeypatch.setenv("LOCAL_RANK", str(r))
        monkeypatch.setattr(local_stack, "_next_port", [0])
        got[r] = [local_stack.free_port() for _ in range(3)]
        assert len(set(got[r])) == 3
    allp = [p for ps in got.values() for p in ps]
    assert len(set(allp)) == len(allp)
    assert all(30000 + 200 * r <= p < 30200 + 200 * r for r, ps in got.items() for p in ps)


def test_bench_tp8_world8():
    """The 70B TP=8 launch form (``torch.distributed.run --nproc-per-node 8 bench.py
    --tp 8``) end to end at world 8 over gloo: rank 0 engine + HTTP stack + load
    generator, ranks 1-7 in the TP worker loop, step inputs over the shared-memory
    ring. CPU-sized model with the 70B head layout (8 kv heads: one per rank)."""
    args = [a if a != "tiny-llama" else "tiny-llama-tp8" for a in ARGS]
    out = _run(_torchrun(8, 29660, args + ["--tp", "8"]))
    assert out["n_gpus"] == 8 and out["config"]["parallelism"] == "tp8" and out["scaling"] == "strong"
    assert out["value"] > 0 and out["p50_ttft_ms"] > 0


@pytest.mark.parametrize("n", [2, 8])
def test_bench_tp_strong_phase(n):
    """the driver's N-rank headline run (DP replicas)
    ALSO serves one model sharded TP=N over the same ranks (the 70B TP=8 config's
    strong-scaling point) and reports it under ``tp_strong`` in the SAME JSON
    line, with the observed process-group backend / world size and the custom
    all-reduce state. Here: gloo, CPU-sized model with 8 kv heads."""
    out = _run(_torchrun(n, 29670 + n, ARGS + ["--full", "--tp-phase", "on", "--tp-model", "tiny-llama-tp8"]))
    assert out["n_gpus"] == n and out["config"]["parallelism"] == f"dp{n}" and out["scaling"] == "weak"
    tp = out["tp_strong"]
    assert tp["status"] == "ok" and tp["model"] == "tiny-llama-tp8" and tp["tp"] == n
    assert tp["pg_world_size"] == n and tp["pg_backend"] == "gloo" and tp["rccl"] is False
    assert tp["custom_allreduce"] is False  # CPU: no IPC collectives
    assert tp["tok_s"] > 0 and tp["p50_ttft_ms"] > 0 and tp["steps"] >= 1
    assert abs(tp["tok_s"] - tp["steps"] * 2 * 4 / (tp["ms_per_step"] * tp["steps"] / 1000)) / tp["tok_s"] < 0.02
    # every rank's start-up breakdown: a TP pod starts as slow as its slowest rank
    per = tp["init_breakdown_s_per_rank"]
    assert isinstance(per, list) and len(per) == n
    assert all(set(r) >= {"weights_s", "collectives_s", "decode_gemm_tune_s", "graph_capture_s"} for r in per)
    assert per[0] == tp["init_breakdown_s"]


def test_bench_tp_phase_time_box():
    """A TP phase that cannot finish in its budget is killed and reported, and the
    headline line is still printed (exit 0)."""
    out = _run([sys.executable, "bench.py"] + ARGS + ["--full", "--tp-phase", "on", "--tp-model", "tiny-llama-tp8",
                                                       "--tp-budget-s", "0.5"])
    assert out["value"] > 0 and out["tp_strong"]["status"] == "timeout"


def test_bench_gpus_flag_must_match_world():
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2"] + ARGS, cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "does not match" in r.stderr


def test_bench_open_loop_request_rate():
    """--request-rate: open-loop Poisson arrivals through the gateway path."""
    out = _run([sys.executable, "bench.py"] + ARGS + ["--request-rate", "20", "--steps", "2"])
    assert out["load"].startswith("open-loop") and out["value"] > 0 and out["p50_ttft_ms"] > 0
    ol = out["open_loop"]
    assert ol["rate_req_s"] == 20 and ol["p90_ttft_ms"] >= ol["p50_ttft_ms"] > 0
    # the tiny CPU model can emit a request's tokens back to back (median gap rounds to 0.00 ms)
    assert ol["p90_itl_ms"] >= ol["p50_itl_ms"] >= 0


def test_bench_tp_strong_rank_failure_fails_fast():
    """VERDICT r5 item 9 (multi-GPU first-run safety): one rank of the world-8 TP phase
    dies while the engines are being built (fault injection: TP rank 3 raises in
    model-runner construction). Every rank must be out within 30 s of the failure
    instead of waiting in a collective for the phase budget, and rank 0 still prints
    the headline line with ``tp_strong.status`` 'failed (exit N)' — not 'timeout'."""
    import time

    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1", HIPSERVE_FAULT="rank3:init@0")
    cmd = _torchrun(8, 29690, ARGS + ["--full", "--tp-phase", "on", "--tp-model", "tiny-llama-tp8",
                                      "--tp-budget-s", "600"])
    t0 = time.time()
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=400)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    tp = lines[0]["tp_strong"]
    assert tp["status"] == "failed (exit 1)", tp
    assert tp["failed_ranks"] == {"3": 1}, tp
    assert lines[0]["value"] > 0  # the headline phase (no TP ranks) was unaffected
    assert tp["phase_wall_s"] < 30, tp  # every rank out within 30 s (3.5 s measured here)
    assert time.time() - t0 < 300


def test_bench_plain_run_has_no_second_phase():
    """Without --full a run is the headline phase alone, whatever --tp-phase says."""
    out = _run([sys.executable, "bench.py"] + ARGS + ["--tp-phase", "on", "--tp-model", "tiny-llama-tp8"])
    assert out["value"] > 0 and out["steps"] == 1 and "tp_strong" not in out


def _dump(tmp_path, name, extra, lo=0):
    import numpy as np

    d = tmp_path / name
    out = _run([sys.executable, "bench.py"] + ARGS + ["--steps", "2", "--dump-outputs", str(d)] + extra)
    assert out["steps"] == 2 and out["ms_per_step"] > 0
    assert sorted(p.name for p in d.iterdir()) == ["tokens.npy"]
    tok = np.load(d / "tokens.npy")
    # one row per request of the last timed wave, one column per generated token
    assert tok.dtype == np.float32 and tok.shape == (2, 4)
    assert ((tok >= lo) & (tok < 512) & (tok == np.round(tok))).all()  # tiny-llama: vocabulary of 512
    return tok


def test_bench_dump_outputs_gateway(tmp_path):
    """--dump-outputs through the gateway path: the ids are read back from the text the
    load generator's clients received (-1: fewer tokens than asked for came back as text,
    or a byte token that is no UTF-8 on its own; half of this tiny vocabulary is byte tokens)."""
    _dump(tmp_path, "gw", [], lo=-1)


def test_bench_dump_outputs_repeatable(tmp_path):
    """Same arguments, same prompts and sampling seeds: the engine path (requests added in
    a fixed order) writes the same tokens in two runs."""
    a = _dump(tmp_path, "a", ["--path", "engine"])
    b = _dump(tmp_path, "b", ["--path", "engine"])
    assert (a == b).all()


def test_bench_ids_from_text_round_trip():
    """The dump reads token ids back from the synthetic tokenizer's text: placeholder
    words, ASCII byte tokens, and a digit byte token right after a word (the merged
    number would exceed the vocabulary)."""
    import bench
    from hipserve.tokenizer import SyntheticTokenizer

    tok = SyntheticTokenizer(512)
    ids = [300, tok.base + ord("7"), 5, 511, tok.base + ord(" "), 400, tok.base + ord("a"), 259]
    assert bench._ids_from_text(tok.decode(ids), tok) == ids
    assert bench._ids_from_text(tok.decode([300, tok.base + 0xC3, 301]), tok) == [300, -1, 301]
