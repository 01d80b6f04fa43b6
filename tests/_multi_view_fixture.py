"""What tests/golden/gen_golden_multi_view.py and tests/test_gpu_multi_view.py share: the form in which multi_view.npz stores the
feature-map gradient."""
import torch


def walsh_rows(C):
    """(C / 4, C) rows of +-1: Walsh functions (-1)^popcount(r & c) of the channel index c, for indices r that span every bit of c"""
    bits = C.bit_length() - 1
    rs = [1 << i for i in range(bits)] + [C - 1]
    r = 3
    while len(rs) < C // 4:
        if r not in rs:
            rs.append(r)
        r += 2
    c = torch.arange(C)
    return torch.stack([1.0 - 2.0 * torch.tensor([bin(int(x) & ri).count("1") % 2 for x in c], dtype=torch.float64) for ri in rs[:C // 4]])
