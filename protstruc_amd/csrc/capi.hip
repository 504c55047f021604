// Library-level entry points of libprotstruc_hip.so (see include/protstruc_hip.h).
// The library keeps no mutable state: there is nothing to initialise, configure or tear down.
#include <hip/hip_runtime.h>

#include "../../include/protstruc_hip.h"

// 2: per-call K1 configuration (ps_k1_config, ps_pairwise_distance_cfg_f32) replaced the process-global
//    ps_set_tuning / ps_get_tuning of version 1.
// 3: ps_k1_plan_f32 (which kernel a K1 launch takes; host-only query); ps_inter_residue_geometry_f32 takes exact_sqrt.
// 4: ps_pairwise_angles_f32 and ps_inter_residue_geometry_f32 take exact_angles (0: fast arithmetic, 1: the reference's
//    order of operations).
// 6: ps_backbone_from_dihedrals_f32 (K7); ps_pointwise_f32 mode 3 (place_fourth_atom).
// 7: ps_backbone_distmat_init_f32 (K8), ps_floyd_warshall_f32 / ps_floyd_warshall_workspace_bytes (K9),
//    ps_backbone_distmat_finish_f32.
// 8: ps_smacof_f32 / ps_smacof_workspace_bytes (K10), ps_mds_backbone_finish_f32 (K11).
// 9: ps_inter_residue_geometry_backward_f32 (the featuriser's vector-Jacobian product).
// 10: ps_backbone_from_dihedrals_backward_f32 (K12, the backbone builder's vector-Jacobian product).
// 11: ps_fape_f32 / ps_fape_backward_f32 (K13 / K14, frame-aligned point error and its gradient),
//     ps_frames_backward_f32 (K4's vector-Jacobian product).
// 12: ps_lddt_f32 / ps_lddt_backward_f32 (K15 / K16, lDDT per point, hard and smooth, and the smooth form's gradient).
// 13: ps_clash_f32 / ps_clash_backward_f32 (K17 / K18, steric clash energy per point and its gradient),
//     ps_peptide_bond_f32 / ps_peptide_bond_backward_f32 (K19 / K20, peptide-bond violations and their gradient).
// 14: ps_backbone_hbonds_f32 (K21, the two best backbone hydrogen bonds of every residue, DSSP energies),
//     ps_dssp_assign (K22, DSSP secondary-structure labels from them).
// 15: ps_solvent_accessibility_f32 (K23, Shrake-Rupley solvent-accessible surface area per point).
// 16: ps_nearest_neighbors_f32 (K24, the k nearest neighbours of every query point, sorted, with masks, keys and a cutoff).
//     Additive to 16 (new symbols change no signature, so the number stays): ps_edge_rbf_f32 (K25, radial basis functions of
//     the atom-pair distances along the edges of a neighbour graph), ps_edge_frames_f32 (K26, the neighbour's frame in the
//     source residue's frame); ps_chi_f32 / ps_chi_backward_f32 (K27 / K28, the side-chain torsions chi1 - chi4 and their
//     gradient), ps_chi_set_f32 / ps_chi_set_backward_f32 (K29 / K30, the side chains turned to given angles, and the
//     gradient towards the angles).
extern "C" int ps_abi_version(void) { return PS_ABI_VERSION; }

extern "C" const char* ps_error_string(int code) { return hipGetErrorString(static_cast<hipError_t>(code)); }

// Always 0: the library contains no timing experiments (the builds that had them are retired; the symbol stays for the ABI)
// and refuses any ps_k1_config with experiment != 0.
extern "C" int ps_has_experiments(void) { return 0; }
