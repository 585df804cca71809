"""The worker side of tools/gpu/optbench.py on the device: the functions every
per-option benchmark script's worker is made of, called in this process for
C2 (-m local) and C3 (-R -m likelihood_ratio) with no option set, at 20,000
sites (one chunk; nothing in these functions depends on the number of chunks),
one warm-up step and one measured step.  The drivers are replayed on the CPU
by test_option_bench.py."""
import hashlib
import types

import pytest

from test_option_bench import ROOT, load

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("config", ["C2", "C3"])
def test_worker_functions(sid, config):
    import torch
    ob = load("optbench")
    a = types.SimpleNamespace(worker=ROOT, config=config, sites=20_000, steps=1, warmup=1)
    cfg, n, text, ln, host, out = ob.worker_start(a, "sets")
    assert n == 20_000 and ln > 0 and out["text_bytes"] == ln and out["sets"] == {}
    assert host.is_pinned() and torch.equal(host, text[:ln].cpu()) and not bool(text[ln:ln + 512].any())
    r = ob.device_pass(a, cfg, text, ln, {})
    assert tuple(r["device_stages_ms"]) == ob.STAGES
    eng, st = ob.pcie_pass(a, cfg, host, ln, n, {}, r)
    digest, newlines = ob.records_digest(eng, st.chunks)
    chunks = list(ob.record_chunks(eng, st.chunks))
    eng.close()
    assert r["device_bytes_out"] == r["pcie_bytes_out"] == sum(len(c) for c in chunks) > 0
    assert r["pcie_chunks"] == st.chunks == len(chunks) and r["device_ms_per_step"] > 0 and r["pcie_ms_per_step"] > 0
    # the same text through a plain engine
    plain = sid.Engine(method=cfg["method"], estimate_prior=cfg["R"])
    plain.source_text(host.numpy().tobytes())
    want, _ = plain.run()
    plain.close()
    assert want.startswith(sid.HEADER)
    assert digest == hashlib.blake2b(want[len(sid.HEADER):]).hexdigest() and newlines == want.count(b"\n") - 1
