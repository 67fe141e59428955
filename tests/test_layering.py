"""The Python binding's module graph, host only:

    native  <-  evaluation  <-  diagnostics  <-  engine
    native  <-  checkpoint                   <-  engine

every relative import of these modules at module level, ``evaluation`` importable without torch,
and ``GameTree.of``: one shared read-only tree per game.
"""
import ast
import os
import subprocess
import sys

import numpy as np
import pytest

import __graft_entry__

EDGES = {
    "native": set(),
    "evaluation": {"native"},
    "checkpoint": {"native"},
    "diagnostics": {"native", "evaluation"},
    "engine": {"native", "checkpoint", "evaluation", "diagnostics"},
}


def relative_imports(module):
    """[(imported sibling module, whether the import is at module level)] of a package module."""
    with open(os.path.join(__graft_entry__.PKG_DIR, module + ".py")) as f:
        tree = ast.parse(f.read())
    top = {id(n) for n in tree.body}
    out = []
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom) and node.level > 0:
            assert node.level == 1, f"{module}: an import from outside the package"
            names = [node.module.split(".")[0]] if node.module else [a.name for a in node.names]
            out += [(name, id(node) in top) for name in names]
    return out


@pytest.mark.parametrize("module", sorted(EDGES))
def test_relative_import_edges(module):
    assert {name for name, _ in relative_imports(module)} == EDGES[module]


@pytest.mark.parametrize("module", ["engine", "evaluation", "diagnostics"])
def test_no_function_local_relative_import(module):
    assert all(at_top for _, at_top in relative_imports(module)), relative_imports(module)


def test_evaluation_imports_without_torch_engine_or_diagnostics():
    code = ("import sys, __graft_entry__\n"
            "pkg = __graft_entry__.load_package()\n"
            "ev = pkg.evaluation\n"
            "assert ev.GameTree.of(1).ndec > 0\n"
            "bad = [m for m in ('torch', 'nfsp_amd.engine', 'nfsp_amd.diagnostics') if m in sys.modules]\n"
            "assert not bad, bad\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=__graft_entry__.REPO, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.parametrize("game", [0, 1])
def test_shared_tree_is_one_read_only_copy(pkg, game):
    GameTree = pkg.evaluation.GameTree
    shared, fresh = GameTree.of(game), GameTree(game)
    assert GameTree.of(game) is shared and shared is not fresh
    arrays = {k: v for k, v in vars(shared).items() if isinstance(v, np.ndarray)}
    assert set(arrays) == {"nodes", "obs", "pay", "lev", "root", "deal", "legal", "seat", "node_of_row"}
    for k, a in arrays.items():
        assert not a.flags.writeable, k
        with pytest.raises(ValueError):
            a[...] = a
        assert a.dtype == getattr(fresh, k).dtype and np.array_equal(a, getattr(fresh, k)), k
        assert getattr(fresh, k).flags.writeable, k
    assert (shared.nn, shared.ndec, shared.nterm, shared.nlev) == (fresh.nn, fresh.ndec, fresh.nterm, fresh.nlev)
    assert shared._rows == fresh._rows
