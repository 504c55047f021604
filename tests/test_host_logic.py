"""Host-side behaviour of the StructureBatch shell (no GPU): constructor
validation, error conventions of the reference, and the absence of
any CPU fallback."""
import numpy as np
import pytest
import torch

from protstruc_amd import ATOM, MAX_N_ATOMS_PER_RESIDUE, StructureBatch


def make(B=2, N=10, A=15, **kw):
    g = torch.Generator().manual_seed(0)
    xyz = torch.randn(B, N, A, 3, generator=g)
    mask = torch.rand(B, N, A, generator=g) < 0.8
    return StructureBatch.from_xyz(xyz, mask, device="cpu", **kw), xyz, mask


def test_atom_enum_matches_reference_slots():
    # reference general.py:4-20
    assert (ATOM.N, ATOM.CA, ATOM.C, ATOM.O, ATOM.CB) == (0, 1, 2, 3, 4)
    assert ATOM["ca"] == ATOM["Ca"] == ATOM["CA"] == 1 and ATOM["cb"] == 4 and ATOM["o"] == 3
    assert ATOM.is_valid("ca") and ATOM.is_valid("CB") and not ATOM.is_valid("CG")
    with pytest.raises(KeyError):
        ATOM["CX"]
    assert MAX_N_ATOMS_PER_RESIDUE == 15


def test_from_xyz_shapes_and_defaults():
    sb, xyz, mask = make()
    assert sb.get_batch_size() == 2 and sb.get_max_n_residues() == 10 and sb.get_max_n_atoms_per_residue() == 15
    assert sb.get_xyz().dtype == torch.float32 and sb.get_xyz().is_contiguous()
    assert torch.equal(sb.residue_mask, mask.any(-1))
    assert sb.chain_idx.shape == (2, 10) and sb.chain_idx.dtype == torch.float32 and (sb.chain_idx == 0).all()
    assert torch.equal(sb.get_residue_mask(), mask[:, :, 1])          # Q5: the getter is the CA slot
    assert sb.get_chain_idx().dtype == torch.long
    assert sb._standardized is False
    # numpy input, no mask, A = 25 as in the reference's own tests (tests/test_StructureBatch.py:11-21)
    sb2 = StructureBatch.from_xyz(np.random.rand(3, 7, 25, 3), device="cpu")
    assert sb2.get_xyz().shape == (3, 7, 25, 3) and sb2.get_xyz().dtype == torch.float32
    assert sb2.residue_mask.all() and sb2.get_atom_mask() is None


def test_chain_arguments_validation():
    xyz = torch.randn(1, 6, 15, 3)
    chain_idx = torch.tensor([[0., 0., 0., 1., 1., 1.]])
    with pytest.raises(ValueError, match="Both `chain_idx` and `chain_ids`"):
        StructureBatch.from_xyz(xyz, chain_idx=chain_idx, device="cpu")
    with pytest.raises(ValueError, match="Both `chain_idx` and `chain_ids`"):
        StructureBatch.from_xyz(xyz, chain_ids=[["A", "B"]], device="cpu")
    with pytest.raises(AssertionError, match="Chain index should start from zero"):
        StructureBatch.from_xyz(xyz, chain_idx=chain_idx + 1, chain_ids=[["A", "B"]], device="cpu")
    padded = torch.tensor([[0., 0., 1., 1., float("nan"), float("nan")]])
    sb = StructureBatch.from_xyz(xyz, chain_idx=padded, chain_ids=[["A", "B"]], device="cpu")
    assert torch.isnan(sb.chain_idx[0, -1])


def test_errors_raised_before_any_launch():
    sb, xyz, mask = make()
    with pytest.raises(ValueError, match="Atom CG is not valid."):
        sb.pairwise_dihedrals(["CA", "CG"], ["CA", "CB"])
    with pytest.raises(KeyError):
        sb.backbone_orientations("N", "CA", "QQ")
    with pytest.raises(KeyError):
        sb.backbone_translations("QQ")
    with pytest.raises(ValueError, match="Only one of atom_mask and residue_mask"):
        sb.standardize(atom_mask=mask, residue_mask=mask.any(-1))
    with pytest.raises(ValueError, match="Cannot unstandardize"):
        sb.unstandardize()
    sb._standardized = True
    with pytest.raises(ValueError, match="already standardized"):
        sb.standardize()


def test_backbone_translations_is_a_view():
    sb, xyz, _ = make()
    t = sb.backbone_translations("N")
    assert torch.equal(t, xyz[:, :, 0]) and t.data_ptr() == sb.get_xyz()[:, :, 0].data_ptr()


@pytest.mark.parametrize("call", [
    lambda sb: sb.pairwise_distance_matrix(),
    lambda sb: sb.backbone_dihedrals(),
    lambda sb: sb.get_n_terminal_mask(),
    lambda sb: sb.backbone_orientations(),
    lambda sb: sb.pairwise_dihedrals(["CA", "CB"], ["CA", "CB"]),
    lambda sb: sb.pairwise_planar_angles(["CA", "CB"], ["CB"]),
    lambda sb: sb.standardize(),
    lambda sb: sb.diffuse_xyz(torch.full((2,), 0.1)),
    lambda sb: sb.inter_residue_geometry(),
])
def test_no_cpu_fallback(call):
    """A CPU-resident batch must raise, never compute on the host."""
    sb, _, _ = make()
    with pytest.raises(RuntimeError, match="HIP-only"):
        call(sb)


# ---- per-device launch settings: one record per device, scoped overrides (host side only: no GPU needed) ----------------
def test_scoped_settings_restore_on_exit_and_after_an_exception():
    from protstruc_amd import _lib
    before = _lib.all_tuning(0)
    with _lib.scoped_settings(0, k1_jt=16, exact_angles=True):
        assert _lib.get_tuning("k1_jt", 0) == 16 and _lib.get_exact_angles(0) == 1
    assert _lib.all_tuning(0) == before and _lib.get_exact_angles(0) == 0
    with pytest.raises(ZeroDivisionError):
        with _lib.scoped_settings(0, k1_rows_per_block=8):
            assert _lib.k1_config(0).rows_per_block == 8
            1 / 0
    assert _lib.all_tuning(0) == before


def test_scoped_settings_nest_and_undo_an_inner_set_tuning():
    from protstruc_amd import _lib, ops
    before = _lib.all_tuning(0)
    with ops.k1_tuning(0, jt=32):
        with ops.k1_tuning(0, jt=64, flat_cpw=2):
            _lib.set_tuning("k1_store_nt", 1, 0)
            _lib.set_exact_angles(True, 0)
            assert (_lib.get_tuning("k1_jt", 0), _lib.get_tuning("k1_flat_cpw", 0), _lib.get_tuning("k1_store_nt", 0)) == (64, 2, 1)
        assert _lib.get_tuning("k1_jt", 0) == 32 and _lib.get_tuning("k1_flat_cpw", 0) == before["k1_flat_cpw"]
        assert _lib.get_tuning("k1_store_nt", 0) == before["k1_store_nt"] and _lib.get_exact_angles(0) == 0
    assert _lib.all_tuning(0) == before


def test_scoped_settings_leave_other_devices_alone():
    from protstruc_amd import _lib
    _lib.all_tuning(1)                                 # device 1's record exists before the scope
    ref1, cfg1 = _lib.k1_config_ref(1), _lib.k1_config(1)
    with _lib.scoped_settings(0, k1_rows_per_block=4, exact_angles=True):
        assert _lib.get_tuning("k1_rows_per_block", 1) == 1 and _lib.get_exact_angles(1) == 0
        assert _lib.k1_config_ref(1) is ref1 and _lib.k1_config(1) is cfg1
    assert _lib.k1_config_ref(1) is ref1


def test_scoped_settings_refuse_an_invalid_value_and_change_nothing():
    from protstruc_amd import _lib, ops
    before, ref = _lib.all_tuning(0), _lib.k1_config_ref(0)
    for bad in ({"k1_jt": 96}, {"k1_rows_per_block": 33}, {"no_such_knob": 1}, {"k1_flat_cpw": 2, "k1_flat": 3}):
        with pytest.raises(_lib.HipLibraryError):
            with _lib.scoped_settings(0, **bad):
                raise AssertionError("the block must not run")
    with pytest.raises(_lib.HipLibraryError):
        with ops.k1_tuning(0, jt=96):
            raise AssertionError("the block must not run")
    assert _lib.all_tuning(0) == before and _lib.k1_config_ref(0) is ref


def test_k1_config_ref_is_cached_until_a_change():
    from protstruc_amd import _lib
    ref, cfg = _lib.k1_config_ref(0), _lib.k1_config(0)
    assert _lib.k1_config_ref(0) is ref and _lib.k1_config(0) is cfg
    assert _lib.k1_config(0, jt=16) is not cfg and _lib.k1_config(0, jt=16).jt == 16 and cfg.jt != 16
    with _lib.scoped_settings(0, k1_jt=16):
        assert _lib.k1_config_ref(0) is not ref and _lib.k1_config(0).jt == 16
        inner = _lib.k1_config_ref(0)
        _lib.set_exact_angles(True, 0)                 # any change installs a new record
        assert _lib.k1_config_ref(0) is not inner
    assert _lib.k1_config_ref(0) is ref and _lib.k1_config(0) is cfg


@pytest.mark.parametrize("var,scope,getter", [("PROTSTRUC_AMD_EXACT_ANGLES", "exact_angles", "get_exact_angles"),
                                              ("PROTSTRUC_AMD_EXACT_SQRT", "exact_sqrt", "get_exact_sqrt")])
def test_leaving_a_scope_gives_back_the_mode_the_environment_selected(var, scope, getter):
    """With the mode switched on through the environment, a ``with ops.exact_...(False)`` block ends in that mode again
    (a fresh child process: the variable is read when a device's record is first built)."""
    import os
    import subprocess
    import sys
    code = ("from protstruc_amd import ops\n"
            f"assert ops.{getter}(0) is True\n"
            f"with ops.{scope}(False, 0):\n"
            f"    assert ops.{getter}(0) is False\n"
            f"assert ops.{getter}(0) is True\n"
            "print('restored')\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, **{var: "1", "PYTHONPATH": root + os.pathsep + os.environ.get("PYTHONPATH", "")})
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd=root, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "restored" in out.stdout, out.stderr
