"""Register / scratch / LDS budget of the temporal history's kernel (csrc/pt_history.h), read from the built libptgpu.so like
tests/test_kernel_resources.py reads the hot kernels'.  The budget is the built value (35 VGPRs) plus a little slack; the
kernel streams: no scratch, no LDS."""
from test_kernel_resources import find, kernel_table


def test_k_hist_advance_stays_within_its_budget(tmp_path):
    k = find(kernel_table(tmp_path), "k_hist_advance")
    assert k["vgpr_count"] <= 40, k
    assert k["private_segment_fixed_size"] == 0 and k["group_segment_fixed_size"] == 0, k
