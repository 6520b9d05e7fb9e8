"""Which kernel family a crypt call runs: the tests' one statement of
plan_crypt's choice (zsummerx_amd/csrc/zrc4_plan.hpp), in plain Python.

Every test that means to reach a family asserts it through these functions, and
three tests hold them against the product: test_family_follows_kernel_class
(tests/test_crypt_plan.py) and test_family_matches_plan_crypt
(tests/test_gpu_addressing.py) against plan_crypt itself through
tools/bin/plan_check, test_kernel_class_follows_launch_crypt
(tests/test_gpu_fused_matrix.py) against the kernels its matrix names.
expected_family of tests/test_gpu_refusals.py is a second statement, written
without this module on purpose.
"""


def kernel_class(mode, first_slot, groups, cus):
    """An in-place "range" or "grouped" call of `groups` groups on `cus` CUs:
    the window kernel up to 32 aligned groups, half-group workgroups while
    2 G <= CUs, whole-group ones while G <= CUs (an unaligned range: gathered
    columns on the whole-group kernel), the persistent kernel above."""
    aligned = mode == "grouped" or first_slot % 256 == 0
    if groups <= 32 and aligned:
        return "win"
    if groups > cus:
        return "stream"
    if 2 * groups <= cus and aligned:
        return "half"
    return "whole"


def family(call, first_slot, n, cus, io=0):
    """The family of a "range", "ids", "grouped" or "declared" call of n
    entries with CryptIo `io`, stated over kernel_class: scattered ids run the
    whole-group kernel up to one group per CU; a rounds call (io = 3) never
    runs the window kernel; declared buckets past the window kernel's 32 run
    crypt_decl_kernel up to one bucket per CU and 256 buckets."""
    G = -(-n // 256)
    if call == "ids":
        return "whole" if G <= cus else "stream"
    aligned = call != "range" or first_slot % 256 == 0
    fam = kernel_class("range" if call == "range" else "grouped", first_slot, G, cus)
    if fam == "win" and io == 3:
        fam = "stream" if G > cus else "half" if 2 * G <= cus and aligned else "whole"
    if call == "declared" and fam in ("half", "whole") and G <= 256:
        fam = "decl"
    return fam


def claim_part(nb, cus, j):
    """The part of a group a declared launch of nb buckets claims for group
    lane j (zrc4_kernels.hpp Claim): the window kernel claims the dword column
    q = col(j) >> 2, the half-group kernel and the persistent kernel (wave-pair
    halves) the half j >> 7, the whole-group kernel the whole group (part 0)."""
    cls = kernel_class("grouped", 0, nb, cus)
    if cls == "win":
        return (j & 31) | ((j >> 7) << 5)
    return j >> 7 if cls in ("half", "stream") else 0


def rounds_groups(which, cus):
    """Group counts of the multi-round range shapes: 1 and 33 the half-group
    kernel (1: where a one-round call takes the window kernel), CUs/2 + 1 the
    whole-group kernel, 257 the host loop over one-round calls."""
    return {"1": 1, "33": 33, "half+1": cus // 2 + 1, "257": 257}[which]
