"""Inputs, configs and stage comparisons shared by the SIFT tests that pin the host layer's per-batch choices (segment
height of the row kernel, octave shapes) and the state kept on the context: test_sift_cases_cpu.py (oracle against the
reference, and the preconditions of the GPU tests), test_gpu_sift_shapes.py, test_gpu_sift_context_state.py.  No tests here."""
import numpy as np

from openpano_amd import synth
from openpano_amd.config import PanoConfig

LOOSE = dict(CONTRAST_THRES=1e-2, PRE_COLOR_THRES=1e-2)
RW_OWN = 240           # columns a band of k_pyramid_rows owns (OP_RW_OWN, csrc/pyramid.hip)


def dense(h, w, seed):
    """uniform noise in [0.25, 0.75), grey: the densest field of DoG extrema there is (test_dense_extrema_fill_the_workgroup_lists)"""
    rng = np.random.default_rng(seed)
    img = np.repeat(rng.random((h, w, 1), dtype=np.float32), 3, axis=2)
    return np.ascontiguousarray(np.float32(0.25) + np.float32(0.5) * img)


def sparse(h, w, seed):
    """blobs on value noise, a few hundred keypoints at these sizes"""
    world = synth.make_world(seed, h + 16, w + 16, work_scale=1.0, density=700.0)
    return np.ascontiguousarray(world[8: 8 + h, 8: 8 + w])


def flat(h, w):
    return np.full((h, w, 3), 0.5, np.float32)


def cfg_for(h, w, **kv):
    """with h + w even the resize ratio is exactly 1: the working image, and so octave 0, has the input's size"""
    assert (h + w) % 2 == 0
    return PanoConfig(SIFT_WORKING_SIZE=(h + w) // 2, **LOOSE, **kv)


def edge_shapes(seg):
    """(h, w) around the seams of k_pyramid_rows at segment height ``seg``: a last segment of seg - 1, seg, 1 and 2 rows
    against a last band of 239, 240, 1 and 2 columns, then a third band of one column and a tall plane of two bands"""
    k = round(240 / seg)
    out = [(h, w) for h in (k * seg - 1, k * seg, k * seg + 1, k * seg + 2) for w in (239, 240, 241, 242) if (h + w) % 2 == 0]
    return out + [(k * seg + 1, 481), (481, 241)]


def shape_seed(h, w):
    return 1000 * h + w


# planes smaller than the kernels' units, all on dense(60, 80, 5): (name, config, descriptors of the oracle)
TINY_IMAGE = (60, 80, 5)
TINY = [
    ("rows_20x27", dict(SIFT_WORKING_SIZE=24), 9),                                          # row kernel, octaves 20x27 down to 8x10
    ("generic6_20x27", dict(SIFT_WORKING_SIZE=24, NUM_SCALE=6), 10),                         # k_pyramid<6>
    ("halo15_5oct", dict(SIFT_WORKING_SIZE=40, GAUSS_WINDOW_FACTOR=10, NUM_OCTAVE=5), 0),    # k_pyramid<0>: halo 15 over a 9x12 plane
    ("rows_13x18_3oct", dict(SIFT_WORKING_SIZE=16, NUM_OCTAVE=3), 3),                        # row kernel, octaves 13x18 down to 7x9
]


def tiny_cfg(kv):
    return PanoConfig(**LOOSE, **kv)


# octave-0 sizes that straddle the 64 x 16 tile of the generic k_pyramid<>
TILE_SHAPES = [(h, w) for h in (95, 96, 97) for w in (127, 128, 129) if (h + w) % 2 == 0]
TILE_CONFIGS = [("scales6", dict(NUM_SCALE=6)), ("window4", dict(GAUSS_WINDOW_FACTOR=4))]

# the context-state sequences (test_gpu_sift_context_state.py) run at one size
SEQ_H, SEQ_W = 241, 481


def seq_images():
    """D1..D3 dense, S / S2 sparse, F flat at 241 x 481; Q1, Q2 dense 240 x 240 (the second size group of one call)"""
    return dict(D1=dense(SEQ_H, SEQ_W, 1), D2=dense(SEQ_H, SEQ_W, 2), D3=dense(SEQ_H, SEQ_W, 3),
                S=sparse(SEQ_H, SEQ_W, 4), S2=sparse(SEQ_H, SEQ_W, 5), F=flat(SEQ_H, SEQ_W),
                Q1=dense(240, 240, 6), Q2=dense(240, 240, 7))


def _compare_stages(g, o, cfg):
    """hip.sift_staged against Oracle.sift_stages: every plane, list and descriptor, bit for bit"""
    assert g.dims == o.dims
    assert np.array_equal(g.work, o.work), "working image"
    for oc in range(cfg.NUM_OCTAVE):
        assert np.array_equal(g.grey[oc], o.gauss[(oc, 0)]), ("grey", oc)
    for kind in ("dog", "mag", "ort"):
        a, b = getattr(g, kind), getattr(o, kind)
        for k in a:
            assert np.array_equal(a[k], b[k]), (kind, k, int((a[k] != b[k]).sum()))
    for k in g.raw:
        assert np.array_equal(g.raw[k], o.raw[k]), ("raw", k)
    for nm in ("refined", "oriented"):
        a, b = getattr(g, nm), getattr(o, nm)
        for f in ("ints", "real", "fl"):
            assert np.array_equal(a[f], b[f]), (nm, f)
    assert np.array_equal(g.desc, o.desc), int((g.desc != o.desc).sum())
    assert np.array_equal(g.coor, o.coor)


def compare_oracle_ref(so, sr):
    """Oracle.sift_stages against Ref.sift_stages, stage by stage (test_oracle_vs_ref.py)"""
    assert so.dims == sr.dims
    assert np.array_equal(so.work, sr.work)
    for kind in ("gauss", "dog", "mag", "ort"):
        a, b = getattr(so, kind), getattr(sr, kind)
        assert a.keys() == b.keys()
        for k in b:
            assert np.array_equal(a[k], b[k]), (kind, k)
    for k in sr.raw:
        assert np.array_equal(so.raw[k], sr.raw[k]), k
    for nm in ("refined", "oriented"):
        a, b = getattr(so, nm), getattr(sr, nm)
        for f in ("ints", "real", "fl"):
            assert np.array_equal(a[f], b[f]), (nm, f)
    assert np.array_equal(so.desc, sr.desc)
    assert np.array_equal(so.coor, sr.coor)


class _Stages:
    pass


def save_stages(path, st):
    """every field of a hip.sift_staged result into one .npz (a child process hands its results to the test this way)"""
    out = dict(work=st.work, dims=np.asarray(st.dims, np.int32), desc=st.desc, coor=st.coor)
    for o, a in st.grey.items():
        out["grey_%d" % o] = a
    for kind in ("dog", "mag", "ort", "raw"):
        for (o, s), a in getattr(st, kind).items():
            out["%s_%d_%d" % (kind, o, s)] = a
    for nm in ("refined", "oriented"):
        for f, a in getattr(st, nm).items():
            out["%s_%s" % (nm, f)] = a
    np.savez(path, **out)


def load_stages(path):
    z = np.load(path)
    st = _Stages()
    st.work, st.desc, st.coor = z["work"], z["desc"], z["coor"]
    st.dims = [tuple(int(v) for v in d) for d in z["dims"]]
    st.grey = {}; st.dog = {}; st.mag = {}; st.ort = {}; st.raw = {}
    st.refined = {}; st.oriented = {}
    for key in z.files:
        kind, _, rest = key.partition("_")
        if kind == "grey":
            st.grey[int(rest)] = z[key]
        elif kind in ("dog", "mag", "ort", "raw"):
            o, s = rest.split("_")
            getattr(st, kind)[(int(o), int(s))] = z[key]
        elif kind in ("refined", "oriented"):
            getattr(st, kind)[rest] = z[key]
    return st


def raw_xy(o, octave=None):
    """raw extrema of an oracle run as one (n, 2) array of x, y (of one octave, or of all)"""
    parts = [np.asarray(v).reshape(-1, 2) for (oc, _), v in o.raw.items() if octave is None or oc == octave]
    return np.concatenate(parts) if parts else np.zeros((0, 2), np.int32)
