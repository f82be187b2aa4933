"""Path parameters of the reference's hydra configs (config/config.yaml, config/category/*.yaml):
only the keys the hot path reads.  load_category_yaml / save_category_yaml read and write the flat form of a category file."""
import dataclasses
import re
from dataclasses import dataclass, field
from typing import List, Optional


@dataclass
class CategoryConfig:
    category: str
    res: float
    vote_range: List[float]
    scale_mean: List[float]
    regress_right: bool
    up_sym: bool = False
    z_right: bool = False
    tr_num_bins: int = 32          # config/config.yaml:7
    rot_num_bins: int = 36         # config/config.yaml:8
    knn: int = 60                  # config/config.yaml:22
    ppffcs: List[int] = field(default_factory=lambda: [84, 32, 32, 16])   # train.py:35
    scale_range: Optional[List[float]] = None   # config/category/*.yaml: the object scale drawn per training view (utils/dataset.py:166)
    npoint_max: int = 10000        # config/config.yaml: views with more points are redrawn (utils/dataset.py:221-222)
    right_sym: bool = False        # config/config.yaml:13; generate_target's right_sym branch (utils/dataset.py:49-50)

    @property
    def out_dim(self):             # train.py:35
        return 2 * self.tr_num_bins + 2 * self.rot_num_bins + 2 + 3


def _c(cat, res, vr, sm, rr, us=False):
    return CategoryConfig(cat, res, [vr, vr], sm, rr, us)


# config/category/{bottle,bowl,camera,can,laptop,mug}.yaml (NOCS) and the SUN RGB-D ones
CATEGORIES = {
    "bottle": _c("bottle", 4e-3, 0.25, [0.05, 0.15, 0.05], False, True),
    "bowl": _c("bowl", 4e-3, 0.12, [0.07, 0.03, 0.07], False),
    "camera": _c("camera", 4e-3, 0.15, [0.05, 0.05, 0.07], True),
    "can": _c("can", 4e-3, 0.1, [0.037, 0.055, 0.037], False, True),
    "laptop": _c("laptop", 1e-2, 0.3, [0.13, 0.1, 0.15], True),
    "mug": _c("mug", 4e-3, 0.12, [0.06, 0.05, 0.045], True, True),
    "bathtub": _c("bathtub", 3e-2, 1.104495769458527, [0.3886107936507936, 0.23178569841269842, 0.6773600634920637], True),
    "bed": _c("bed", 3e-2, 1.860647331329598, [1.0274129618644066, 0.49417050423728714, 0.7768076129943503], True),
    "bookshelf": _c("bookshelf", 3e-2, 1.501261827212904, [0.2166509734042553, 0.8096084361702133, 0.6821934095744682], True, True),
    "chair": _c("chair", 3e-2, 0.7863312261283193, [0.29636475108453486, 0.4208450279047945, 0.2789450356430997], True),
    "sofa": _c("sofa", 3e-2, 1.5296381674297101, [0.48090147859327237, 0.4228677186544341, 0.9288330076452599], True),
    "table": _c("table", 3e-2, 1.2363029403529906, [0.4305247031772566, 0.35199163168896463, 0.6905431275083608], True),
}
NOCS_CATEGORIES = ["bottle", "bowl", "camera", "can", "laptop", "mug"]   # nocs/inference.py synset order


# config/category/*.yaml:scale_range (training views only, cppf_amd/meshes.py)
_SCALE_RANGE = {
    "bottle": [0.2300, 0.4594], "bowl": [0.1851, 0.2381], "camera": [0.1430, 0.2567], "can": [0.128, 0.18],
    "laptop": [0.3862, 0.5353], "mug": [0.1501, 0.1995],
    "bathtub": [0.9871392690983584, 2.3263480392772227], "bed": [1.484997764725992, 4.096944229262802],
    "bookshelf": [0.1640900157049736, 4.339695465933739], "chair": [0.7999364364268209, 1.559057241958137],
    "sofa": [0.7900343820741655, 3.7988801202149647], "table": [0.027254089050664287, 3.6816547320083073],
}
for _cat, _sr in _SCALE_RANGE.items():
    CATEGORIES[_cat].scale_range = _sr


# ----------------------------------------------------------------------------------------------------------------- YAML files
# config/config.yaml's values of the keys a category file may leave out (a category file is composed over it)
YAML_DEFAULTS = dict(res=5e-3, npoint_max=10000, regress_right=False, tr_num_bins=32, rot_num_bins=36, up_sym=False, right_sym=False,
                     z_right=False, knn=60)
_YAML_KEYS = ("category", "res", "up_sym", "right_sym", "z_right", "regress_right", "vote_range", "scale_mean", "scale_range",
              "tr_num_bins", "rot_num_bins", "knn", "npoint_max")
_INT = re.compile(r"^[-+]?[0-9]+$")
_FLOAT = re.compile(r"^[-+]?(\d+\.?\d*|\.\d+)([eE][-+]?\d+)?$")


def _scalar(text):
    t = text.strip()
    if len(t) >= 2 and t[0] == t[-1] and t[0] in "'\"":
        return t[1:-1]
    if t in ("True", "true", "TRUE", "yes", "Yes", "on", "On"):
        return True
    if t in ("False", "false", "FALSE", "no", "No", "off", "Off"):
        return False
    if t in ("null", "Null", "NULL", "~", ""):
        return None
    if _INT.match(t):
        return int(t)
    if _FLOAT.match(t):
        return float(t)
    return t


def parse_flat_yaml(text):
    """The top-level `key: value` pairs of a flat YAML file such as config/category/*.yaml: scalars (numbers like 4e-3 are floats,
    unlike YAML 1.1), inline lists `[a, b]` and booleans.  Nested blocks (`opt:`, `hydra:`, `defaults:` ...), their indented lines
    and comments (`# @package _global_`) are skipped.  Not a YAML parser: anything beyond this form raises or is skipped."""
    out = {}
    for ln, raw in enumerate(text.splitlines(), 1):
        if not raw.strip() or raw.lstrip().startswith("#") or raw[0] in " \t-":
            continue
        line = re.sub(r"\s+#.*$", "", raw).rstrip()
        if ":" not in line:
            raise ValueError(f"line {ln}: not a `key: value` pair: {raw!r}")
        key, val = line.split(":", 1)
        key, val = key.strip(), val.strip()
        if not val:
            continue                                                  # a nested block follows
        if val.startswith("["):
            if not val.endswith("]"):
                raise ValueError(f"line {ln}: an inline list must close on its line: {raw!r}")
            body = val[1:-1].strip()
            out[key] = [_scalar(x) for x in body.split(",")] if body else []
        else:
            out[key] = _scalar(val)
    return out


def load_category_yaml(path, defaults=None):
    """A CategoryConfig from a category file in the flat form of config/category/*.yaml, over config/config.yaml's defaults
    (YAML_DEFAULTS, or `defaults`: a dict or the path of such a file).  Keys that are not CategoryConfig fields (max_epoch, opt,
    hydra, batch_size ...) are ignored.  The file must give category, vote_range and scale_mean."""
    base = dict(YAML_DEFAULTS)
    if isinstance(defaults, str):
        defaults = parse_flat_yaml(open(defaults).read())
    base.update({k: v for k, v in (defaults or {}).items() if k in _YAML_KEYS})
    vals = parse_flat_yaml(open(path).read())
    base.update({k: v for k, v in vals.items() if k in _YAML_KEYS})
    missing = [k for k in ("category", "vote_range", "scale_mean") if k not in base]
    if missing:
        raise ValueError(f"{path}: no {', '.join(missing)}")
    base["category"] = str(base["category"])
    for k in ("res",):
        base[k] = float(base[k])
    for k in ("vote_range", "scale_mean", "scale_range"):
        if base.get(k) is not None:
            base[k] = [float(x) for x in base[k]]
    for k in ("tr_num_bins", "rot_num_bins", "knn", "npoint_max"):
        base[k] = int(base[k])
    for k in ("up_sym", "right_sym", "z_right", "regress_right"):
        if not isinstance(base[k], bool):
            raise ValueError(f"{path}: {k} must be True or False, not {base[k]!r}")
    return CategoryConfig(**base)


def save_category_yaml(cfg, path):
    """Write `cfg` in the flat form of config/category/*.yaml (every key load_category_yaml reads; floats as repr, so a load gives
    the same values back)."""
    d = dataclasses.asdict(cfg)
    fmt = lambda v: repr(float(v)) if isinstance(v, float) else str(v)
    lines = ["# @package _global_"]
    for k in _YAML_KEYS:
        v = d.get(k)
        if v is None:
            continue
        lines.append(f"{k}: [{', '.join(fmt(float(x)) for x in v)}]" if isinstance(v, (list, tuple)) else f"{k}: {fmt(v)}")
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
