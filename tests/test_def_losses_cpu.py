"""The index-matched losses on the deformed region (MLSP/mlsp.py:184-427) are part of the public surface: the shim exports all
five with the reference's signatures, and the library exports their entry points.  Runs without a GPU."""
import inspect
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAMES = ("findindexs", "findneareat_index", "calc_def_normal_loss", "calc_def_density_loss", "deform_densityloss")
# the reference's parameter lists (MLSP/mlsp.py:184, 196, 289, 331, 370), kept here so the test also runs where the reference is absent
REF_PARAMS = {
    "findindexs": ["pred", "gold", "mask"],
    "findneareat_index": ["p1", "p2", "mask"],
    "calc_def_normal_loss": ["args", "logits", "normal_labels", "mask", "indexes", "device", "all"],
    "calc_def_density_loss": ["args", "logits", "density_labels", "mask", "indexes", "device", "criterion", "all"],
    "deform_densityloss": ["args", "logits", "density_labels", "density_mse_label", "mask", "indexes", "device"],
}
SYMBOLS = ("mlsp_def_nearest_index_f32", "mlsp_def_normal_loss_fwd_f32", "mlsp_def_normal_loss_bwd_f32", "mlsp_def_density_loss_fwd_f32",
           "mlsp_def_density_loss_bwd_f32", "mlsp_gather_rows_u32", "mlsp_gather_rows_bwd_f32")


def _shim_mlsp():
    shims = os.path.join(ROOT, "mlsp_amd", "shims")
    if shims not in sys.path:
        sys.path.insert(0, shims)
    from MLSP import mlsp
    assert mlsp.__file__.startswith(shims), mlsp.__file__
    return mlsp


def test_shim_exports_the_def_losses():
    mlsp = _shim_mlsp()
    for name in NAMES:
        assert hasattr(mlsp, name), name
        assert list(inspect.signature(getattr(mlsp, name)).parameters) == REF_PARAMS[name], name
    sig = inspect.signature(mlsp.calc_def_normal_loss)
    assert sig.parameters["all"].default is False
    assert inspect.signature(mlsp.calc_def_density_loss).parameters["all"].default is False


def test_signatures_match_the_reference():
    """inspect.signature of each against the reference itself (imported through tools/ref_import.py where it exists)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import ref_import
    if not os.path.isdir(ref_import.REF_ROOT):
        pytest.skip("reference not present")
    _, _, ref_mlsp = ref_import.import_reference()
    from mlsp_amd import mlsp
    for name in NAMES:
        ref_sig = inspect.signature(getattr(ref_mlsp, name))
        assert list(ref_sig.parameters) == REF_PARAMS[name], name
        ours = inspect.signature(getattr(mlsp, name))
        assert [(p.name, p.default) for p in ours.parameters.values()] == \
            [(p.name, p.default) for p in ref_sig.parameters.values()], name


def test_library_exports_the_def_loss_entry_points():
    from mlsp_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built here")
    lib = _lib.load()
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert lib.mlsp_abi_version() == 14


def test_def_losses_have_no_cpu_fallback():
    import torch
    from mlsp_amd import _lib, mlsp
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built here")
    with pytest.raises(_lib.MlspLibraryError):
        mlsp.findindexs(torch.zeros(1, 8, 3), torch.zeros(1, 3, 8), torch.ones(1, 3, 8))
