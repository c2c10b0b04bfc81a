"""What tests/test_gpu_clip_tables.py relies on, from the oracle alone (oracle/trimmomatic_oracle.py on
the CPU): on the pairs of tests/clip_table_cases.py every test of ILLUMINACLIP fires often enough on
every table, and every rule the table shapes exercise decides answers, so a kernel that agrees with
the oracle on these pairs has run the rule.

Measured (300 pairs a table, seed 5): pairs with a palindrome hit, hits of each prefix pair, reads 1 /
reads 2 clipped by a simple-mode adapter, reads 2 dropped.

  table                spec              palindrome  per pair         simple1  simple2  dropped2
  simple_only          :0:90:10:0:true            -  -                    120      128         9
  simple_only          :2:30:10                   -  -                    128      141        12
  simple_only          :1:30:7:1:false            -  -                    147      154        12
  prefix_only          :0:90:10:0:true            9  9                      -        -         0
  prefix_only          :2:30:10                  76  76                     -        -        76
  prefix_only          :1:30:7:1:false           78  78                     -        -        78
  unequal_long_prefix  :0:90:10:0:true           29  29                    74       58        26
  unequal_long_prefix  :2:30:10                  78  78                    75       66       107
  unequal_long_prefix  :1:30:7:1:false           77  77                    82       75       109
  roles                :0:90:10:0:true            7  7                     52       31         3
  roles                :2:30:10                  63  63                    55       35        67
  roles                :1:30:7:1:false           63  63                    63       39        69
  full                 :0:90:10:0:true           20  0, 0, 3, 17           46       45        22
  full                 :2:30:10                  62  19, 15, 13, 24        49       52        88
  full                 :1:30:7:1:false           62  19, 15, 13, 24        56       61        89

The default spec's palindrome threshold of 90 asks for 150 matching bases, which a prefix pair of 12 to
20 bases reaches only with a fragment of 110 bases or more, so the floors per prefix pair and the
witnesses of the prefix rules are asserted under the two specs with a threshold of 30.

Witnesses: reads (of both mates) whose keep length changes when the oracle loses one rule, under
:0:90:10:0:true / :2:30:10 / :1:30:7:1:false.

  roles ignored (every adapter common)   roles 45 / 47 / 54, full 39 / 44 / 51
  prefixes cut from their 5' ends        unequal_long_prefix 58 / 134 / 134, full 6 / 14 / 14
  the first prefix pair only             full 40 / 86 / 86
  the last prefix pair only              full 6 / 75 / 75
  the adapters' last 16-mer not packed   (named cases) simple_only 28 / 28 / 32 of 32 reads,
                                         unequal_long_prefix 32 / 32 / 32 of 32, roles 14 / 14 / 16 of 16,
                                         full 75 / 75 / 88 of 88; under :1:30:7:1:false the oracle drops
                                         every one of them and the variant keeps every one whole
  the palindrome walk's ref one base low (named cases of full, the 17 / 20 pair) 12 / 12 / 12; the 300
                                         drawn pairs change nowhere, which is why the cases are built
"""
import pytest

from tests import clip_table_cases as cc

THRESHOLD_30 = [":2:30:10", ":1:30:7:1:false"]
WITNESS_MIN = 10
WITH_ADAPTERS = [t for t in cc.TABLES if cc.adapters(t)]
WITH_PREFIXES = [t for t in cc.TABLES if cc.prefix_pairs(t)]


@pytest.fixture(scope="module")
def fasta_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("clip_tables")


def test_the_tables_are_the_shapes():
    from crispresso_amd.trim import TrimOptions

    shapes = {}
    for t in cc.TABLES:
        o = TrimOptions()
        o.set_adapters(cc.records(t))
        shapes[t] = ([len(p1) for p1, _ in o.prefix_pairs], sorted((len(a), r) for a, r in o.adapters))
    assert shapes["simple_only"] == ([], [(24, 0), (25, 0), (27, 0), (28, 0)])
    assert shapes["prefix_only"] == ([34], [])
    assert shapes["unequal_long_prefix"] == ([58], [(31, 0), (39, 0), (58, 0), (61, 0)])
    assert shapes["roles"] == ([20], [(30, 1), (33, 2), (40, 0)]) and len(cc.adapters("roles")) == 4
    pre, ads = shapes["full"]
    assert pre == [12, 16, 17, 128] and [n for n, _ in ads] == sorted(cc.FULL_ADAPTERS)
    assert sorted(r for _, r in ads) == [0] * 6 + [1] * 5 + [2] * 5
    assert [cc.seeds_of(n) for n in (24, 27, 28, 128)] == [3, 3, 4, 29]
    assert cc.SPECS == [":0:90:10:0:true", ":2:30:10", ":1:30:7:1:false"]


def test_the_files_parse_alike(fasta_dir):
    """The oracle and the package read the same roles, prefix pairs and duplicates out of each file."""
    from crispresso_amd.trim import TrimOptions

    for t in cc.TABLES:
        path = cc.write_fasta(t, fasta_dir)
        clip = cc.tmo.IlluminaClip(path + cc.SPECS[2])
        o = TrimOptions.from_steps("ILLUMINACLIP:" + path + cc.SPECS[2])
        assert [(pp.p1.encode(), pp.p2.encode()) for pp in clip.pairs] == o.prefix_pairs
        theirs = [(cs.seq.encode(), role) for role, group in ((1, clip.fwd), (2, clip.rev), (0, clip.com))
                  for cs in group]
        assert theirs == o.adapters
        assert all(cs.min_overlap == 11 for cs in clip.fwd + clip.rev + clip.com)


def test_pairs_are_the_kinds():
    for t in cc.TABLES:
        plist = cc.pairs(t)
        assert len(plist) == cc.N_PAIRS and plist == cc.pairs(t)
        lens = [len(p[i]) for p in plist for i in (0, 2)]
        assert min(lens) >= 8 and max(lens) == 151
        assert all(len(p[0]) == len(p[1]) and len(p[2]) == len(p[3]) for p in plist)
        assert all(len(p[0]) == len(p[2]) == 151 for p in plist[0::6])
        quals = [max(max(p[1]), max(p[3])) - 33 for p in plist]
        assert max(quals) == 93 and max(q for k, q in enumerate(quals) if k % 5 != 4) == 41
        assert min(min(p[1]) for p in plist) == 33


@pytest.mark.parametrize("spec", cc.SPECS)
@pytest.mark.parametrize("table", cc.TABLES)
def test_the_oracle_fires(table, spec, fasta_dir):
    _, _, c = cc.oracle(table, spec, fasta_dir)
    print(table, spec, c)
    if table in WITH_ADAPTERS:
        assert c["simple1"] >= 30 and c["simple2"] >= 30
    if table in WITH_PREFIXES:
        if spec in THRESHOLD_30:
            assert c["palindrome"] >= 50 and min(c["per_pair"]) >= 5
        else:
            assert c["palindrome"] >= 5
    else:
        assert c["palindrome"] == 0
    if not cc.tmo.IlluminaClip(cc.write_fasta(table, fasta_dir) + spec).keep_both:
        assert c["dropped2"] >= 5


def witness(table, spec, directory, variant, what="pairs"):
    n = cc.changed(cc.oracle(table, spec, directory, what), cc.oracle(table, spec, directory, what, variant=variant))
    print(variant.__name__, table, spec, what, n)
    return n


@pytest.mark.parametrize("table,spec", [("roles", s) for s in cc.SPECS] + [("full", cc.SPECS[0]), ("full", cc.SPECS[2])])
def test_witness_roles(table, spec, fasta_dir):
    assert witness(table, spec, fasta_dir, cc.variant_roles_ignored) >= WITNESS_MIN


@pytest.mark.parametrize("table,spec", [("unequal_long_prefix", s) for s in cc.SPECS] + [("full", cc.SPECS[2])])
def test_witness_prefix_cut_from_the_3prime_ends(table, spec, fasta_dir):
    assert witness(table, spec, fasta_dir, cc.variant_cut_5prime) >= WITNESS_MIN


@pytest.mark.parametrize("variant", [cc.variant_first_pair_only, cc.variant_last_pair_only])
def test_witness_every_prefix_pair(variant, fasta_dir):
    assert witness("full", cc.SPECS[2], fasta_dir, variant) >= WITNESS_MIN


@pytest.mark.parametrize("table", WITH_ADAPTERS)
def test_witness_last_seed_of_every_adapter(table, fasta_dir):
    """Every adapter (and role) of the table has its four reads that only its last 16-mer seeds."""
    cases = cc.named(table)
    carriers = [(i, m, len(p[2 * (m - 1)])) for i, (label, mates, p) in enumerate(cases) if label == "last16"
                for m in mates]
    roles = {ar for ar in cc.adapters(table)}
    assert len(carriers) == sum(4 * (2 if role == 0 else 1) for _, role in roles)
    for spec in cc.SPECS:
        assert witness(table, spec, fasta_dir, cc.variant_no_last_seed, "named") >= WITNESS_MIN
    full = cc.oracle(table, cc.SPECS[2], fasta_dir, "named")
    less = cc.oracle(table, cc.SPECS[2], fasta_dir, "named", variant=cc.variant_no_last_seed)
    assert all(full[m - 1][i] == 0 for i, m, _ in carriers)
    assert all(less[m - 1][i] == n for i, m, n in carriers)


def test_named_heads_seed_below_the_minimum_overlap_only(fasta_dir):
    """Adapter heads of 12 to 15 bases at the 3' end: clipped under the threshold-7 spec (minimum overlap
    11), left whole where the minimum overlap is 15."""
    for table in WITH_ADAPTERS:
        cases = cc.named(table)
        heads = [(i, m, len(p[2 * (m - 1)])) for i, (label, mates, p) in enumerate(cases) if label == "head"
                 for m in mates]
        low = cc.oracle(table, cc.SPECS[2], fasta_dir, "named")
        high = cc.oracle(table, cc.SPECS[0], fasta_dir, "named")
        assert len(heads) >= 16
        assert all(n - 15 <= low[m - 1][i] <= n - 12 for i, m, n in heads)
        assert all(high[m - 1][i] == n for i, m, n in heads)


@pytest.mark.parametrize("spec", cc.SPECS)
def test_witness_palindrome_walk(spec, fasta_dir):
    """`ref` one base low at every step of a prefix pair with an odd number of skipped steps (the
    17 / 20 pair of full): each spec has its six built pairs, both mates of which change."""
    cases = cc.named("full")
    walk = [i for i, (label, _, _) in enumerate(cases) if label == "walk"]
    assert len(walk) == 18
    assert witness("full", spec, fasta_dir, cc.variant_walk_shifted, "named") >= WITNESS_MIN
    a = cc.oracle("full", spec, fasta_dir, "named")
    b = cc.oracle("full", spec, fasta_dir, "named", variant=cc.variant_walk_shifted)
    assert {i for i in range(len(cases)) if a[0][i] != b[0][i] or a[1][i] != b[1][i]} <= set(walk)


def test_long_cases(fasta_dir):
    plist = cc.long_cases()
    assert [len(p[i]) for p in plist for i in (0, 2)] == [4096] * 4
    for spec in cc.SPECS:
        k1, k2, c = cc.oracle("full", spec, fasta_dir, "long")
        assert c["palindrome"] == 1 and c["per_pair"][-1] == 1 and c["simple1"] + c["simple2"] == 1
        assert k1[0] == cc.LONG_FRAGMENT and sorted((int(k1[1]), int(k2[1]))) == [4000, 4096]
