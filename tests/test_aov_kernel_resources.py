"""Register / scratch / LDS budgets of the AOV kernels (csrc/pt_aov.h), read from the built libptgpu.so like
tests/test_kernel_resources.py reads the hot kernels'.  The budgets are the built values plus a little slack."""
from test_kernel_resources import find, kernel_table

# variant <ALPHA, GRID> -> (VGPRs, scratch bytes per lane); the KD variants' scratch is next_hit's traversal stack
K_AOV = {"ILb0ELb1EE": (116, 0), "ILb1ELb1EE": (164, 0), "ILb0ELb0EE": (140, 1312), "ILb1ELb0EE": (200, 1312)}
K_AOV_SAMPLES = {"ILb0ELb1EE": (64, 0), "ILb1ELb1EE": (116, 0), "ILb0ELb0EE": (88, 1312), "ILb1ELb0EE": (148, 1312)}


def test_aov_kernels_stay_within_their_budgets(tmp_path):
    t = kernel_table(tmp_path)
    for kernel, budgets in (("5k_aov", K_AOV), ("13k_aov_samples", K_AOV_SAMPLES)):
        for variant, (vgprs, scratch) in budgets.items():
            k = find(t, f"_Z{kernel}{variant}")
            assert k["vgpr_count"] <= vgprs and k["private_segment_fixed_size"] <= scratch, (kernel, variant, k)
            assert k["group_segment_fixed_size"] == 0, (kernel, variant, "the reduction is cross-lane: no LDS")
    g = find(t, "k_aov_guides")
    assert g["vgpr_count"] <= 40 and g["private_segment_fixed_size"] == 0 and g["group_segment_fixed_size"] == 0, g
