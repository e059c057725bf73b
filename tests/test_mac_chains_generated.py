"""csrc/mac_chains.inc is generated: re-running tools/gen_mac_chains.py must reproduce the committed file exactly."""
from tools import gen_mac_chains


def test_mac_chains_inc_matches_generator():
    with open(gen_mac_chains.output_path()) as f:
        committed = f.read()
    assert gen_mac_chains.render() == committed, "mac_chains.inc is stale: run python3 tools/gen_mac_chains.py"


def test_fused_columns_cover_every_mac_once():
    # every a[i]*b[j] (i + j = k) and every m[i]*p[j] with p[j] != 0, j >= 1 appears in column k exactly once
    p = gen_mac_chains.FUSED_FIELDS["Stark252"]
    n = len(p)
    for k in range(2 * n - 1):
        text = gen_mac_chains.fused_col("Stark252", p, k)
        ab = sum(1 for i in range(n) if 0 <= k - i < n)
        mp = sum(1 for i in range(min(k, n)) if 1 <= k - i < n and p[k - i] != 0)
        assert text.count("v_mad_u64_u32") == ab + mp, k
        assert f"{ab} a*b + {mp} m*p MACs" in text
