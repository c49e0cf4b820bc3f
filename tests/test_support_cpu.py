"""CPU: the test-support layer (tests/support.py) -- no file under tests/ or tools/ imports a test module, and same_bits compares
shape, dtype and every bit, on NumPy arrays and on CPU tensors."""
import ast
import glob
import os

import numpy as np
import pytest

import support
from conftest import ROOT


def test_no_file_imports_a_test_module():
    """helpers that two test files need live in the helper module of their subject, never in one of the two"""
    found = []
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "**", "*.py"), recursive=True) + glob.glob(os.path.join(ROOT, "tools", "*.py"))):
        with open(path) as f:
            tree = ast.parse(f.read(), path)
        for node in ast.walk(tree):
            names = ([a.name for a in node.names] if isinstance(node, ast.Import) else
                     [node.module or ""] if isinstance(node, ast.ImportFrom) else [])
            found += ["%s:%d imports %s" % (os.path.relpath(path, ROOT), node.lineno, n) for n in names
                      if any(part.startswith("test_") for part in n.split("."))]
    assert found == []


def nan(payload):
    """a float64 quiet NaN with the given payload bits"""
    return np.array([0x7FF8000000000000 | payload], np.uint64).view(np.float64)[0]


# (a, b, the same bits)
CASES = {
    "equal": (np.array([[1.5, -2.0], [0.0, 3.25]]), np.array([[1.5, -2.0], [0.0, 3.25]]), True),
    "value": (np.array([1.0, 2.0]), np.array([1.0, np.nextafter(2.0, 3.0)]), False),
    "shape": (np.zeros((2, 3)), np.zeros((3, 2)), False),
    "dtype": (np.array([1.0, 2.0], np.float32), np.array([1.0, 2.0], np.float64), False),
    "signed zero": (np.array([0.0, 1.0]), np.array([-0.0, 1.0]), False),
    "nan payloads": (np.array([nan(1), 1.0]), np.array([nan(2), 1.0]), False),
    "same nan": (np.array([nan(1), 1.0]), np.array([nan(1), 1.0]), True),
    "float32 signed zero": (np.array([0.0], np.float32), np.array([-0.0], np.float32), False),
    "complex equal": (np.array([1 + 2j, complex(nan(3), -0.0)]), np.array([1 + 2j, complex(nan(3), -0.0)]), True),
    "complex imaginary zero": (np.array([complex(1.0, 0.0)]), np.array([complex(1.0, -0.0)]), False),
    "complex nan payloads": (np.array([complex(0.0, nan(1))]), np.array([complex(0.0, nan(2))]), False),
    "int32 equal": (np.array([1, -2, 3], np.int32), np.array([1, -2, 3], np.int32), True),
    "int32 value": (np.array([1, -2, 3], np.int32), np.array([1, -2, 4], np.int32), False),
    "int32 against int64": (np.array([1, 2], np.int32), np.array([1, 2], np.int64), False),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_same_bits_numpy(name):
    a, b, same = CASES[name]
    assert support.same_bits(a, b) is same and support.same_bits(b, a) is same
    assert support.same_bits(a, a.copy()) and support.same_bits(b, b.copy())


@pytest.mark.parametrize("name", sorted(CASES))
def test_same_bits_tensors(name):
    import torch
    a, b, same = (torch.from_numpy(x) if isinstance(x, np.ndarray) else x for x in CASES[name])
    assert support.same_bits(a, b) is same and support.same_bits(b, a) is same
    assert support.same_bits(a, a.clone()) and support.same_bits(b, b.clone())


def test_same_bits_takes_views():
    """a strided view is compared by its values, not by the memory it lies in"""
    import torch
    x = np.arange(12.0).reshape(3, 4)
    assert support.same_bits(x[:, 1], np.array([1.0, 5.0, 9.0])) and not support.same_bits(x[:, 1], x[:, 2])
    t = torch.from_numpy(x)
    assert support.same_bits(t[:, 1], torch.tensor([1.0, 5.0, 9.0], dtype=torch.float64)) and not support.same_bits(t[:, 1], t[:, 2])
    z = torch.from_numpy(np.array([[1 + 2j, 3 - 4j], [5j, 6.0]]))
    assert support.same_bits(z[:, 0], torch.from_numpy(np.array([1 + 2j, 5j])))
