"""CPU: the bootstrap replicates of `python -m shannon_amd.quant -b B --seed S`.  The brute force of rule 1
(tests/bootstrap_cases.py) against the generator's known answers, a hand-checked input and its own numpy form; the host parts of the
feature: abundance.bootstrap_summary, the texts of the two new files, and the command's argument checks."""
import math
import numpy as np
import pytest
import bootstrap_cases as bc


# ---------------------------------------------------------------------------------------------------------------- the brute force
def test_philox_known_answers():
    for counter, key, want in bc.KNOWN_ANSWERS:
        assert bc.philox(counter, key) == want


def test_brute_force_on_a_hand_checked_input():
    """N = 3, classes of 2 and 1 fragments (cum 0, 2, 3), seed 0.  Replicate 0: u = 0xe169c58d6627e8d5 (the first known answer's o0 and
    o1), 0x5cb200dbf8e4cca4, 0x51c732a604faa329 -- 0.880, 0.362 and 0.319 of 2^64, times 3: r = 2, 1, 0, classes 1, 0, 0.  Replicate 1: u =
    0xea23..., 0xe4c2..., 0x86d2... -- 0.915, 0.894, 0.527: r = 2, 2, 1, classes 1, 1, 0."""
    o = bc.philox((0, 0, 0, 0), (0, 0))
    assert o[0] | o[1] << 32 == 0xe169c58d6627e8d5
    assert [bc.draw(t, 0, 0, 3) for t in range(3)] == [2, 1, 0]
    assert [bc.draw(t, 1, 0, 3) for t in range(3)] == [2, 2, 1]
    cum = bc.cum_of([2, 1])
    assert cum == [0, 2, 3] and [bc.class_of(cum, r) for r in (0, 1, 2)] == [0, 0, 1]
    assert bc.brute_counts([2, 1], 2, 0) == [[2, 1], [1, 2]]


def test_brute_force_sums_and_empty_classes():
    for n_c, B, seed in (([5, 0, 3], 4, 7), ([0, 0, 9, 0], 3, 0), ([40, 25], 3, (1 << 64) - 1), ([1], 2, 5), ([0, 0], 2, 1)):
        counts = bc.brute_counts(n_c, B, seed)
        assert all(sum(row) == sum(n_c) for row in counts)
        assert all(row[c] == 0 for row in counts for c, n in enumerate(n_c) if n == 0)
        assert np.array_equal(bc.brute_counts_np(n_c, B, seed), np.array(counts, dtype=np.uint64).reshape(B, len(n_c)))
    assert bc.brute_counts([40, 25], 2, 7) != bc.brute_counts([40, 25], 2, 8)                  # the seed is used
    assert bc.brute_counts([40, 25], 2, 7) != bc.brute_counts([40, 25], 2, 7 + (1 << 32))      # ... and so is its high word
    rows = bc.brute_counts([40, 25], 3, 7)
    assert rows[0] != rows[1] and rows[:2] == bc.brute_counts([40, 25], 2, 7)                  # a replicate does not depend on B


def test_resample_cases_are_what_they_say():
    cases = bc.resample_cases()
    assert sum(cases["64 draws"]) == 64 and sum(cases["65 draws"]) == 65 and cases["an empty class between two"][1] == 0
    big = cases["1,000 random classes, N = 10,000"]
    assert len(big) == 1000 and sum(big) == 10000
    few = cases["5,000 classes, N = 200"]
    assert len(few) == 5000 and sum(few) == 200 and sum(1 for n in few if n == 0) > 4700
    assert sum(cases["no fragments"]) == 0
    for n in (8192, 8193):
        many = cases["%s classes, N = 6,703" % format(n, ",")]
        assert len(many) == n and sum(many) == 6703 and many[17] >= 6000 and many[-1] >= 3


# ---------------------------------------------------------------------------------------------------------------- the summary
def direct_summary(rows):
    B, out = len(rows), []
    for j in range(len(rows[0])):
        xs = [rows[b][j] for b in range(B)]
        mean = 0.0
        for x in xs:
            mean += x
        mean /= B
        ss = 0.0
        for x in xs:
            ss += (x - mean) * (x - mean)
        out.append((mean, math.sqrt(ss / (B - 1)) if B > 1 else 0.0, min(xs), max(xs)))
    return out


def test_bootstrap_summary():
    from shannon_amd import abundance
    rng = np.random.Generator(np.random.PCG64(5))
    for B, m in ((1, 4), (2, 3), (7, 5), (100, 2)):
        rows = (rng.uniform(0.0, 1e4, (B, m)) * (rng.uniform(0, 1, (B, m)) > 0.2)).tolist()
        got = abundance.bootstrap_summary(rows)
        want = direct_summary(rows)
        assert list(zip(got["bs_mean"], got["bs_sd"], got["bs_min"], got["bs_max"])) == want
        assert abundance.bootstrap_summary(np.array(rows)) == got                 # a matrix or lists
        if B == 1:
            assert got["bs_sd"] == [0.0] * m and got["bs_mean"] == rows[0] == got["bs_min"] == got["bs_max"]
    # by hand: 1, 2, 6 -> mean 3, squared distances 4 + 1 + 9 = 14, sd sqrt(7)
    got = abundance.bootstrap_summary([[1.0], [2.0], [6.0]])
    assert got == {"bs_mean": [3.0], "bs_sd": [math.sqrt(7.0)], "bs_min": [1.0], "bs_max": [6.0]}
    with pytest.raises(ValueError):
        abundance.bootstrap_summary([])


# ---------------------------------------------------------------------------------------------------------------- the texts
TABLE = {"names": ["tA", "tB"], "length": [300, 1200], "eff_length": [101.5, 1001.25], "est_counts": [10.0, 0.1], "tpm": [250000.0, 750000.0],
         "bs_est_counts": [[9.5, 0.0], [11.0, 0.5]], "bs_tpm": [[1e6, 0.0], [400000.0, 600000.0]], "bs_rounds": [50, 100],
         "bs_mean": [10.25, 0.25], "bs_sd": [1.0606601717798212, 0.3535533905932738], "bs_min": [9.5, 0.0],
         "bs_max": [11.0, 0.5]}


def test_text_of_a_replicate_and_of_the_summary():
    from shannon_amd import abundance
    assert abundance.abundance_tsv(abundance.replicate_table(TABLE, 0)) == ("target_id\tlength\teff_length\test_counts\ttpm\n"
                                                                            "tA\t300\t101.5\t9.5\t1000000.0\n"
                                                                            "tB\t1200\t1001.25\t0.0\t0.0\n")
    assert abundance.abundance_tsv(abundance.replicate_table(TABLE, 1)) == ("target_id\tlength\teff_length\test_counts\ttpm\n"
                                                                            "tA\t300\t101.5\t11.0\t400000.0\n"
                                                                            "tB\t1200\t1001.25\t0.5\t600000.0\n")
    assert abundance.bootstrap_summary_tsv(TABLE) == ("target_id\test_counts\tbs_mean\tbs_sd\tbs_min\tbs_max\n"
                                                      "tA\t10.0\t10.25\t1.0606601717798212\t9.5\t11.0\n"
                                                      "tB\t0.1\t0.25\t0.3535533905932738\t0.0\t0.5\n")
    s = abundance.bootstrap_summary(TABLE["bs_est_counts"])
    assert all(s[k] == TABLE[k] for k in s)


# ---------------------------------------------------------------------------------------------------------------- the command
@pytest.fixture()
def base(tmp_path):
    fa, r = tmp_path / "t.fasta", tmp_path / "r.fa"
    fa.write_text(">a\nACGTACGTACGTACGTACGT\n")
    r.write_text(">0\nACGTACGTACGTACGTACGT\n")
    return ["quant", str(fa), "-o", str(tmp_path / "OUT"), "--single", str(r)]


def test_parse_args_accepts_b_and_seed(base):
    from shannon_amd import quant
    o = quant.parse_args(base)
    assert isinstance(o, dict) and "bootstraps" not in o and "seed" not in o
    o = quant.parse_args(base + ["-b", "1"])
    assert o["bootstraps"] == 1 and "seed" not in o
    o = quant.parse_args(base + ["-b", "100", "--seed", "18446744073709551615"])
    assert o["bootstraps"] == 100 and o["seed"] == (1 << 64) - 1
    o = quant.parse_args(base[:1] + ["--seed", "0", "-b", "3"] + base[1:])
    assert o["bootstraps"] == 3 and o["seed"] == 0
    assert "-b B" in quant.USAGE and "--seed S" in quant.USAGE and "-b B" in quant.__doc__ and "--seed S" in quant.__doc__


@pytest.mark.parametrize("extra, message", [(["-b", "0"], "-b 0 is outside"), (["-b", "2.5"], "-b 2.5 is not an integer"),
                                            (["-b", "x"], "-b x is not an integer"), (["--seed", "5"], "--seed belongs to -b"),
                                            (["-b", "2", "--seed", "-1"], "--seed -1 is outside"),
                                            (["-b", "2", "--seed", "18446744073709551616"], "--seed 18446744073709551616 is outside"),
                                            (["-b", "2", "--seed", "1e3"], "--seed 1e3 is not an integer"),
                                            (["-b", "1", "-b", "2"], "-b given twice"), (["-b", "2", "--seed", "1", "--seed", "2"], "--seed given twice"),
                                            (["-b"], "-b needs a value"), (["-b", "4294967296"], "-b 4294967296 is outside")])
def test_main_refuses_bad_b_and_seed(base, capsys, extra, message):
    from shannon_amd import quant
    assert isinstance(quant.parse_args(base + extra), str)
    capsys.readouterr()
    assert quant.main(base + extra) == 2                          # (refused before the device is touched)
    err = capsys.readouterr().err
    assert message in err and "usage:" in err
