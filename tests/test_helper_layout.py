"""Test modules are not libraries: what tests, scripts and oracle tools share lives in plain helper modules (builders.py,
gpu_util.py, sharp_refs.py, sampler_refs.py, decoder_refs.py, mlp_refs.py, loss_refs.py, adam_refs.py, grad_edge_refs.py, scan_refs.py, actor_refs.py, table_grad_refs.py, proposal_refs.py, raygen_refs.py, composite_refs.py, plugin_harness.py, host_gate.py, synth.py, the restatements), so that editing
a test cannot break a tool or another test."""
import ast
import glob
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_no_file_imports_a_test_module():
    files = [f for d in ("tests", "scripts", "oracle") for f in glob.glob(os.path.join(ROOT, d, "**", "*.py"), recursive=True)]
    assert len(files) > 50
    bad = []
    for f in files:
        for node in ast.walk(ast.parse(open(f).read(), f)):
            mods = [a.name for a in node.names] if isinstance(node, ast.Import) else \
                [node.module or ""] if isinstance(node, ast.ImportFrom) else []
            bad += [(os.path.relpath(f, ROOT), node.lineno, m) for m in mods if any(p.startswith("test_") for p in m.split("."))]
    assert not bad, bad
