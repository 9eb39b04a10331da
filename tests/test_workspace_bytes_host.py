"""The workspace / scratch sizes the library asks for are pinned: every size entry point over the table of
tools/dump_workspace_bytes.py against tests/golden/workspace_bytes.json (that tool's output).  Host arithmetic: no device needed."""
import importlib.util
import json
import os

from tests.helpers import REPO
from tests.test_abi_symbols import lib_path  # noqa: F401  (fixture)


def _dump_tool():
    spec = importlib.util.spec_from_file_location("dump_workspace_bytes", os.path.join(REPO, "tools", "dump_workspace_bytes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_workspace_bytes_match_golden(lib_path):  # noqa: F811
    with open(os.path.join(REPO, "tests", "golden", "workspace_bytes.json")) as f:
        golden = json.load(f)
    rows = _dump_tool().dump(lib_path)
    assert len(golden) == 324
    assert [(r["entry"], r["args"]) for r in rows] == [(r["entry"], r["args"]) for r in golden]
    for got, want in zip(rows, golden):
        assert got["bytes"] == want["bytes"], (want["entry"], want["args"], got["bytes"], want["bytes"])
