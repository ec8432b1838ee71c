"""The small and lopsided nets -- what the planner chooses only there (tests/test_small_nets_cpu.py, tests/test_small_nets_gpu.py).

idc_create takes any net whose height and width are positive multiples of 8.  Below 32 x 48 the planner leaves the paths every other test
walks: a click launch on at most three site rows is the one-wave conv_click<T,1,1> (set_geometry shrinks wp while 4 * wp > 2 * Hs), conv1_2 of
an operand-split or fp16 handle stays on the 64-cout <1,4> tile (its grid never reaches the 256 workgroups of conv1_2_split_kernel), and an
fp32 max_batch-32 handle on 16 x 264 takes conv_igemm<f32,1,4> for conv1_1 and, without Winograd, for conv1_2.  GRID is the list of such
configurations, declared once: the CPU census plans every one of them with tools/plan_dump and holds each conv label against the exact tables,
the GPU file runs forwards on its nets.

A helper, not a conftest: nothing here touches the library or a GPU."""
import collections
import subprocess

import fused_head_ref
import model1_ref
from test_ops_exact_gpu import CASES, normalise
from test_plan_cpu import FLAG_BITS

PRECISIONS = ("fp32", "bf16", "bf16x3", "bf16x6", "fp16x3", "fp16")
NETS = ((8, 8), (8, 16), (16, 8), (24, 24), (8, 136), (136, 8))      # (H, W): a 1 x 1, 1 x 2, 2 x 1, 3 x 3, 1 x 17 and 17 x 1 trunk
WIDE_NET = (16, 264)                                                 # nine 32-wide tile columns on two trunk rows
SIX_PRECISION_NETS = ((8, 8), (8, 136), (136, 8))                    # where the GPU file runs all six precisions (fp32 and bf16 elsewhere)
MAX_BATCHES = (1, 32)
# the options that take a precision off its default batch-1 kernels (fp32: Winograd, bf16: K over the waves) and leave conv_click in their place
OPTIONS = {"fp32": ((), (("winograd", 0),)), "bf16": ((), (("kwave", 0),))}
DIST_PRECISIONS = ("fp32", "bf16", "fp16x3")                         # the 529-bin head: the precisions test_ops_exact_gpu.SHIPPED builds

Config = collections.namedtuple("Config", "precision flags H W max_batch options")      # flags: names of FLAG_BITS; options: (name, value) pairs


def _grid():
    """Per (net, max_batch, precision): no flag under each option set of the precision, dist313 under the defaults, dist under the defaults on
    DIST_PRECISIONS; the wide net in fp32 and bf16 only.  The heads' layers hang off conv8_3 and the hyper-columns: a flag adds rows to a plan
    and changes none, so the option sets are crossed with the flag-free plan alone."""
    out = []
    for H, W in NETS + (WIDE_NET,):
        for mb in MAX_BATCHES:
            for p in PRECISIONS if (H, W) != WIDE_NET else ("fp32", "bf16"):
                for opts in OPTIONS.get(p, ((),)):
                    out.append(Config(p, (), H, W, mb, opts))
                out.append(Config(p, ("dist313",), H, W, mb, ()))
                if p in DIST_PRECISIONS:
                    out.append(Config(p, ("dist",), H, W, mb, ()))
    return out


GRID = _grid()
assert len(set(GRID)) == len(GRID)

# Rows of a layer table that are no conv launch, by the kernel column (a prefix): the regression head and the softmax of the distribution
# heads are kernels of their own (tests/test_heads_gpu.py), "fused into ..." marks a layer that rides in another one's launch (the consumer's
# row is the launch), and the first row of every table stands for the input pack, which conv1_1's operand staging builds.
NOT_A_CONV = ("head_kernel", "softmax_nchw_kernel", "fused into ", "(input pack fused into conv1_1)")

# The exact rows this census asked for (tests/test_ops_exact_gpu.py): taken out of the covered set they leave the census with UNREACHED_BEFORE.
NEW_ROW_IDS = (
    "f32_click11_d2_1x1px", "f32_click11_3x17", "f32_click11_d2_3x3", "f32_click11_deconv_resid", "f32_click11_384_resid",
    "bf16_click11_d2_1x1px", "bf16_click11_3x17", "bf16_click11_d2_3x3", "bf16_click11_deconv_resid", "bf16_click11_f32resid_384",
    "bf16x3_v2ps_14", "bf16x6_v2ps_14", "fp16x3_v2psh_14", "fp16_v2psh_14", "f32_igemm_14_16x264", "bf16x3_v2s_22_halo2_small",
)
UNREACHED_BEFORE = {
    "conv_click<f32,1,1>", "conv_click<bf16,1,1>", "conv_igemm_v2ps<1,4>x3", "conv_igemm_v2ps<1,4>x6", "conv_igemm_v2psh<1,4>x3",
    "conv_igemm_v2psh<1,4>x1", "conv_igemm<f32,1,4>",
    # an eighth, which the list this census started from had missed: the dilated trunk (conv5_1 .. conv6_3) of a small bf16x3 net under the
    # default options.  The table held conv_igemm_v2s<2,2>x6 and conv_igemm_v2sh<2,2>x3, and this label only with '+head' (fused_head_ref).
    "conv_igemm_v2s<2,2>x3",
}


def describe(cfg):
    return "%d x %d %s max_batch %d%s%s" % (cfg.H, cfg.W, cfg.precision, cfg.max_batch, "".join(" " + f for f in cfg.flags),
                                            "".join(" %s=%d" % kv for kv in cfg.options))


def plan_rows(plan_dump, cfg):
    """The layer table tools/plan_dump prints for a configuration (n = 1: the variant follows max_batch), as layer_table() rows."""
    cmd = [plan_dump, cfg.precision, str(sum(FLAG_BITS[f] for f in cfg.flags)), str(cfg.H), str(cfg.W), str(cfg.max_batch), "1"]
    cmd += ["%s=%d" % kv for kv in cfg.options]
    out = subprocess.check_output(cmd, text=True)
    return [dict(name=n, kernel=k, launches=int(l)) for n, k, l in (line.split("\t") for line in out.splitlines())]


def family(label):
    """A label's family with its template arguments: no ' splitK<n>', and none of the run-time suffixes plan_dump does not print (the exact
    table says 'conv_ds_fused_m+shortcut 8-wave' and '... half', the dump 'conv_ds_fused_m+shortcut')."""
    return normalise(label)


def covered(without=()):
    """The families a row of an exact table reaches: test_ops_exact_gpu.CASES (less the ids in `without`), model1_ref.ROWS (both of a row's
    labels), fused_head_ref.ROWS.  Rows that need the -DIDC_AB_PARTNERS build do not count.  A '+head' row reaches '+head' labels only:
    it runs conv10_2 under a tolerance and never stores it, which says nothing about the plain kernel of the same name."""
    out = set(family(c.label) for c in CASES if not c.partner and c.id not in without)
    for r in model1_ref.ROWS:
        if not r.partner:
            out.update(family(k) for k in (r.conv1_1, r.conv1_2))
    out.update(family(r.label) for r in fused_head_ref.ROWS)
    return out


def conv_rows(rows):
    for r in rows:
        k = r["kernel"]
        if any(k.startswith(p) for p in NOT_A_CONV):
            continue
        assert k.startswith("conv") and r["launches"] > 0, "a row that is neither a conv launch nor on the list of what is not: %r" % (r,)
        yield r


def census(plans, reached):
    """plans: [(Config, rows)].  {family: (configuration, layer) of the first plan that launches it} for every conv label outside `reached`."""
    out = collections.OrderedDict()
    for cfg, rows in plans:
        for r in conv_rows(rows):
            f = family(r["kernel"])
            if f not in reached and f not in out:
                out[f] = (describe(cfg), r["name"])
    return out
