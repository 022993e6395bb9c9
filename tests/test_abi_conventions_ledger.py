"""The ledger of the calling-convention tests: every function of include/mvf.h that takes a ``void* stream`` is covered by a
GPU test in each of the three modes of ``tests/_kernel_scaffold.convention`` - on a side stream behind in-flight inputs, at
displaced pointers, with its ``const`` inputs checked for change - or stands in the table below with the reason why not.

The test modules are read with ``ast``, not imported (no test module imports another one, and none of them needs a GPU to be
read): each declares ``CONVENTION_COVERS = {"mvf_name": ("side_stream", "displaced", "inputs"), ...}`` (``MODES``: all three)
next to a parametrised test over those entry points and modes.  An entry point added to the header fails here until a module
covers it."""
import ast
import pathlib
import re

ROOT = pathlib.Path(__file__).resolve().parents[1]
MODES = ("side_stream", "displaced", "inputs")

# entry point -> (modes left out, why): argued exemptions
EXEMPT = {
    "mvf_allreduce_stats": (MODES, "multi-GPU exchange: runs on a side stream of its own in tests/test_gpu_rccl.py, one process per rank"),
    "mvf_assign": (("displaced",), "its operands are a prepared case of HipKernels allocations (tests/_align_kernel_scaffold.py)"),
    "mvf_assign_dense": (("displaced",), "its operands are a prepared case of HipKernels allocations"),
    "mvf_assign_topk": (("displaced",), "its operands are a prepared case of HipKernels allocations"),
    "mvf_assign_best": (("displaced",), "its operands are a prepared case of HipKernels allocations"),
    "mvf_assign_apply": (("displaced",), "its operands are a prepared case of HipKernels allocations"),
    "mvf_assign_layer_stats": (("displaced",), "its layer is prepared by the device when the case is built (tests/test_gpu_align_start_kernels.py)"),
    "mvf_rhs_cached": (("displaced",), "reads the cache and the operands that HipKernels built (tests/test_gpu_wide.py)"),
    "mvf_apply_cached": (("displaced",), "reads the cache and the operands that HipKernels built (tests/test_gpu_wide.py)"),
}


def stream_functions():
    """Names of the functions of include/mvf.h with a ``void* stream`` parameter."""
    text = re.sub(r"/\*.*?\*/", " ", (ROOT / "include" / "mvf.h").read_text(), flags=re.S)
    found = []
    for m in re.finditer(r"\b(mvf_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S):
        if re.search(r"\bvoid\s*\*\s*stream\b", m.group(2)):
            found.append(m.group(1))
    return found


def declared_covers():
    """{entry point: {mode: [modules]}} from the CONVENTION_COVERS of every tests/test_gpu_*.py."""
    covers = {}
    for path in sorted((ROOT / "tests").glob("test_gpu_*.py")):
        for node in ast.parse(path.read_text()).body:
            if not (isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "CONVENTION_COVERS" for t in node.targets)):
                continue
            assert isinstance(node.value, ast.Dict), f"{path.name}: CONVENTION_COVERS must be a dict display"
            for key, value in zip(node.value.keys, node.value.values):
                name = ast.literal_eval(key)
                if (isinstance(value, ast.Name) and value.id == "MODES") or (isinstance(value, ast.Attribute) and value.attr == "MODES"):
                    modes = MODES
                else:
                    modes = tuple(ast.literal_eval(value))
                assert set(modes) <= set(MODES), (path.name, name, modes)
                for mode in modes:
                    covers.setdefault(name, {}).setdefault(mode, []).append(path.name)
            src = path.read_text()
            assert "under(" in src and "parametrize(\"mode\"" in src, f"{path.name} declares coverage without a test over the modes"
    return covers


def test_the_header_is_parsed():
    names = stream_functions()
    assert len(names) == len(set(names)) >= 64, len(names)
    for known in ("mvf_read_back", "mvf_gram_cached", "mvf_solve_minnorm_lrd_async", "mvf_mesh_loss", "mvf_heat_graph", "mvf_kde"):
        assert known in names, known
    for without in ("mvf_version", "mvf_debug_option", "mvf_comm_create", "mvf_gram_workspace_bytes", "mvf_assign_padded_features"):
        assert without not in names, without


def test_every_entry_point_is_covered_in_every_mode_or_stands_in_a_table_with_its_reason():
    names, covers = stream_functions(), declared_covers()
    unknown = sorted(set(covers) - set(names))
    assert not unknown, f"CONVENTION_COVERS names no function of include/mvf.h with a stream: {unknown}"
    missing = []
    for name in names:
        left_out = set(EXEMPT.get(name, ((), ""))[0])
        for mode in MODES:
            if mode not in covers.get(name, {}) and mode not in left_out:
                missing.append(f"{name}: {mode}")
    assert not missing, "entry points without a convention test:\n  " + "\n  ".join(missing)


def test_the_table_holds_nothing_stale():
    names, covers = stream_functions(), declared_covers()
    for name, (modes, reason) in EXEMPT.items():
        assert name in names, f"{name} is not in include/mvf.h any more"
        assert modes and set(modes) <= set(MODES) and reason.strip(), name
        for mode in modes:
            assert mode not in covers.get(name, {}), f"{name}: {mode} is covered by {covers[name][mode]}; drop the exemption"
