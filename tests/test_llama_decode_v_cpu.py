"""tools/llama_decode.py --v: the model-level decode tool builds its VQuantLinear layers with vector length 8 (default) or 16 -
the 1.4 - 1.6 bit formats (v16-k65536-1024 / -256 / -64) were out of its reach.  Host logic, no GPU."""
import importlib.util
import inspect
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("llama_decode_tool", os.path.join(ROOT, "tools", "llama_decode.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_build_model_takes_the_vector_length():
    ld = _tool()
    p = inspect.signature(ld.build_model).parameters
    assert "v" in p and p["v"].default == 8
    src = inspect.getsource(ld.build_model)
    assert "vector_lens=[-1, v]" in src and "vector_lens=[-1, 8]" not in src


def test_command_line_offers_v_8_and_16(monkeypatch, capsys):
    import runpy
    path = os.path.join(ROOT, "tools", "llama_decode.py")
    monkeypatch.setattr(sys, "argv", ["llama_decode.py", "--help"])
    with pytest.raises(SystemExit) as e:
        runpy.run_path(path, run_name="__main__")
    assert e.value.code == 0
    assert "--v {8,16}" in capsys.readouterr().out
    monkeypatch.setattr(sys, "argv", ["llama_decode.py", "--v", "12"])
    with pytest.raises(SystemExit) as e:      # (argparse turns another vector length down before anything touches a GPU)
        runpy.run_path(path, run_name="__main__")
    assert e.value.code == 2
