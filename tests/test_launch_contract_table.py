"""Every launching entry point of include/protstruc_hip.h is held to the launch contract by some GPU test (no GPU needed
here): it is either in the case table of tests/launch_cases.py, which tests/test_gpu_launch_contract.py runs on a side
stream, inside a captured graph and from four threads, or in HELD_ELSEWHERE below, which names the older test that
captures it.  A kernel added later fails here until it is in one of the two."""
import os
import re

import torch

from tests import launch_cases
from tests.c_headers import declared_symbols

TESTS = os.path.dirname(os.path.abspath(__file__))

K1 = "tests.test_gpu_parity::test_k1_capi_argument_validation_streams_and_capture"
K3 = "tests.test_gpu_parity::test_k3_inside_a_captured_graph"
K5 = "tests.test_gpu_parity::test_k5_graph_capture_replays_fresh_noise"
NERF = "tests.test_gpu_nerf::test_graph_capture"
NERF_BACKWARD = "tests.test_gpu_nerf_backward::test_inside_a_captured_graph"
IRG_BACKWARD = "tests.test_gpu_irg_backward::test_inside_a_captured_graph"
DISTMAT = "tests.test_gpu_distmat::test_graph_capture"
MDS = "tests.test_gpu_mds::test_deterministic_and_graph_capture"
# the tests that held an entry point to the capture contract before the case table existed: the only values allowed below
OLDER_TESTS = (K1, K3, K5, NERF, NERF_BACKWARD, IRG_BACKWARD, DISTMAT, MDS)

# launcher -> the older test whose captured graph contains it
HELD_ELSEWHERE = {
    "ps_pairwise_distance_f32": K1,            # the C entry point called directly ...
    "ps_pairwise_distance_cfg_f32": K1,        # ... and through ops.pairwise_distance, which passes the device's configuration
    "ps_pairwise_angles_f32": K3,
    "ps_inter_residue_geometry_f32": K3,
    "ps_diffuse_f32": K5,                      # StructureBatch.diffuse_xyz ...
    "ps_frames_f32": K5,                       # ... and .backbone_orientations in the same graph
    "ps_backbone_from_dihedrals_f32": NERF,
    "ps_backbone_from_dihedrals_backward_f32": NERF_BACKWARD,
    "ps_inter_residue_geometry_backward_f32": IRG_BACKWARD,
    "ps_backbone_distmat_init_f32": DISTMAT,   # geometry.reconstruct_backbone_distmat_from_interresidue_geometry: all three
    "ps_floyd_warshall_f32": DISTMAT,
    "ps_backbone_distmat_finish_f32": DISTMAT,
    "ps_smacof_f32": MDS,
}

# host-only symbols: queries, plans and defaults that launch nothing
DOES_NOT_LAUNCH = ("ps_abi_version", "ps_has_experiments", "ps_error_string", "ps_k1_config_default", "ps_k1_plan_f32",
                   "ps_k3_plan_f32", "ps_featuriser_plan_f32", "ps_floyd_warshall_workspace_bytes", "ps_smacof_workspace_bytes")


def test_every_launcher_is_held_to_the_launch_contract():
    declared = set(declared_symbols("protstruc_hip.h"))
    in_table = set(launch_cases.symbols())
    assert in_table <= declared, f"the case table names symbols the header does not declare: {sorted(in_table - declared)}"
    assert set(HELD_ELSEWHERE) <= declared and set(DOES_NOT_LAUNCH) <= declared
    assert not in_table & set(DOES_NOT_LAUNCH) and not set(HELD_ELSEWHERE) & set(DOES_NOT_LAUNCH)
    missing = declared - in_table - set(HELD_ELSEWHERE) - set(DOES_NOT_LAUNCH)
    assert not missing, (f"{sorted(missing)}: add a case to tests/launch_cases.py (tests/test_gpu_launch_contract.py then runs it "
                         "on a side stream, in a captured graph and from four threads)")


def test_the_older_tests_exist_and_capture():
    assert set(HELD_ELSEWHERE.values()) <= set(OLDER_TESTS)
    for test_id in OLDER_TESTS:
        module, name = test_id.split("::")
        source = open(os.path.join(TESTS, module.split(".")[1] + ".py")).read()
        found = re.search(rf"^def {name}\(.*?(?=^def |\Z)", source, flags=re.S | re.M)
        assert found, f"{test_id} is gone: move its launchers into tests/launch_cases.py"
        assert "torch.cuda.graph(" in found.group(0), f"{test_id} captures no graph any more"


def test_the_case_table_is_well_formed():
    names = [case.name for case in launch_cases.CASES]
    assert len(set(names)) == len(names)
    for case in launch_cases.CASES:
        assert case.symbols and callable(case.build) and callable(case.run), case.name
        a, b = case.build("A"), case.build("B")
        assert list(a) == list(b) and set(case.strided) <= set(a), case.name
        converted = bool(case.strided)
        for key in a:
            assert a[key].shape == b[key].shape and a[key].dtype == b[key].dtype, (case.name, key)
            converted |= a[key].dtype in (torch.float64, torch.int64) or (key.endswith("mask") and a[key].is_floating_point())
        assert converted, f"{case.name}: no input forces a conversion in the shell"
        assert any(not same_bits(a[key], b[key]) for key in a), f"{case.name}: the two variants are the same"
        again = case.build("A")
        assert all(same_bits(a[key], again[key]) for key in a), f"{case.name}: the builder is not seeded"


def same_bits(x, y):
    return torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))

