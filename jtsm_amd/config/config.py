"""CfgNode / get_cfg — the configuration front door of the reference (detectron2/config/config.py:12-113
on top of yacs/fvcore, neither of which is in the reference tree or this image): attribute-style nested
dict, `_BASE_` inheritance between YAML files, `merge_from_file`, `merge_from_list`, freeze/defrost.

Only the keys the JTSM path reads carry defaults (jtsm_amd/config/defaults.py).  Unlike yacs, merging a
file may introduce keys that have no default: the reference's YAMLs set many options of subsystems that
are out of scope here (solver, datasets, test-time augmentation), and they must still load unchanged.
"""
import ast
import copy
import os

import yaml

BASE_KEY = "_BASE_"
EVAL_TAG = "tag:yaml.org,2002:python/object/apply:eval"

_BINARY = {ast.Add: lambda a, b: a + b, ast.Sub: lambda a, b: a - b, ast.Mult: lambda a, b: a * b,
           ast.Div: lambda a, b: a / b, ast.Pow: lambda a, b: a ** b}


def eval_arithmetic(text):
    """The value of a `!!python/object/apply:eval` string (Base-RetinaNet.yaml writes its anchor sizes as one), without
    eval: the expression's AST may hold numeric literals, lists and tuples, + - * / **, unary minus, and ONE list
    comprehension over a literal list with the name(s) it binds.  The operators are Python's own on Python's own
    numbers, so the doubles are the ones eval gives.  Anything else — a call, an attribute, a subscript, a string, a
    name that was not bound — raises ValueError."""
    if not isinstance(text, str) or len(text) > 1000:
        raise ValueError("config: the eval tag takes one short string")
    try:
        tree = ast.parse(text.strip(), mode="eval")
    except SyntaxError as e:
        raise ValueError("config: cannot parse %r: %s" % (text, e)) from None
    state = {"comprehensions": 0}

    def number(v):
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise ValueError("config: %r is not a number" % (v,))
        return v

    def walk(node, names):
        if isinstance(node, ast.Constant):
            return number(node.value)
        if isinstance(node, (ast.List, ast.Tuple)) and isinstance(node.ctx, ast.Load):
            items = [walk(e, names) for e in node.elts]
            return items if isinstance(node, ast.List) else tuple(items)
        if isinstance(node, ast.Name) and isinstance(node.ctx, ast.Load) and node.id in names:
            return names[node.id]
        if isinstance(node, ast.UnaryOp) and isinstance(node.op, ast.USub):
            return -number(walk(node.operand, names))
        if isinstance(node, ast.BinOp) and type(node.op) in _BINARY:
            a, b = number(walk(node.left, names)), number(walk(node.right, names))
            if isinstance(node.op, ast.Pow) and (abs(b) > 64 or abs(a) > 1e6):
                raise ValueError("config: %r ** %r is out of the range an anchor size needs" % (a, b))
            return _BINARY[type(node.op)](a, b)
        if isinstance(node, ast.ListComp):
            state["comprehensions"] += 1
            gen = node.generators[0]
            if state["comprehensions"] > 1 or len(node.generators) != 1 or gen.ifs or gen.is_async \
                    or not isinstance(gen.iter, (ast.List, ast.Tuple)):
                raise ValueError("config: one list comprehension over a literal list, no conditions")
            targets = [gen.target] if isinstance(gen.target, ast.Name) else getattr(gen.target, "elts", [None])
            if not all(isinstance(t, ast.Name) for t in targets):
                raise ValueError("config: a comprehension binds plain names")
            out = []
            for item in walk(gen.iter, {}):                       # (a literal: it sees no names)
                bound = dict(names)
                if isinstance(gen.target, ast.Name):
                    bound[gen.target.id] = item
                else:
                    if not isinstance(item, (list, tuple)) or len(item) != len(targets):
                        raise ValueError("config: cannot unpack %r" % (item,))
                    bound.update({t.id: v for t, v in zip(targets, item)})
                out.append(walk(node.elt, bound))
            return out
        raise ValueError("config: %s is not allowed in an eval tag (%r)" % (type(node).__name__, text))

    return walk(tree.body, {})


class _Loader(yaml.SafeLoader):
    """yaml.SafeLoader plus the one python tag the reference's configs use."""


def _construct_eval(loader, node):
    if not isinstance(node, yaml.SequenceNode) or len(node.value) != 1 or not isinstance(node.value[0], yaml.ScalarNode):
        raise yaml.constructor.ConstructorError(None, None, "the eval tag takes a list of one string", node.start_mark)
    try:
        return eval_arithmetic(loader.construct_scalar(node.value[0]))
    except ValueError as e:
        raise yaml.constructor.ConstructorError(None, None, str(e), node.start_mark) from None


_Loader.add_constructor(EVAL_TAG, _construct_eval)


class CfgNode(dict):
    def __init__(self, init_dict=None):
        super().__init__()
        self.__dict__["_frozen"] = False
        for k, v in (init_dict or {}).items():
            self[k] = CfgNode(v) if isinstance(v, dict) and not isinstance(v, CfgNode) else self._decode(v)

    @staticmethod
    def _decode(v):
        """YAML keeps python literals such as `(60000, 80000)` as strings; evaluate them like yacs does."""
        if isinstance(v, str):
            try:
                return ast.literal_eval(v)
            except (ValueError, SyntaxError):
                return v
        return v

    # attribute access ---------------------------------------------------------------------------
    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None

    def __setattr__(self, name, value):
        if self.__dict__.get("_frozen", False):
            raise AttributeError("Attempted to set {} to {}, but CfgNode is immutable".format(name, value))
        self[name] = value

    # yacs-like API -------------------------------------------------------------------------------
    def freeze(self):
        self._set_frozen(True)

    def defrost(self):
        self._set_frozen(False)

    def is_frozen(self):
        return self.__dict__["_frozen"]

    def _set_frozen(self, flag):
        self.__dict__["_frozen"] = flag
        for v in self.values():
            if isinstance(v, CfgNode):
                v._set_frozen(flag)

    def clone(self):
        return copy.deepcopy(self)

    def __deepcopy__(self, memo):
        out = CfgNode()
        for k, v in self.items():
            dict.__setitem__(out, k, copy.deepcopy(v, memo))
        out.__dict__["_frozen"] = self.__dict__["_frozen"]
        return out

    def dump(self, **kwargs):
        def plain(n):
            return {k: plain(v) if isinstance(v, CfgNode) else (list(v) if isinstance(v, tuple) else v)
                    for k, v in n.items()}
        return yaml.safe_dump(plain(self), **kwargs)

    @staticmethod
    def _coerce(new, old):
        """Keep the declared type where a YAML literal is a near miss (tuple vs list, int vs float)."""
        if old is None or new is None or type(new) is type(old):
            return new
        if isinstance(old, tuple) and isinstance(new, list):
            return tuple(new)
        if isinstance(old, list) and isinstance(new, tuple):
            return list(new)
        if isinstance(old, float) and isinstance(new, int):
            return float(new)
        if isinstance(old, (list, tuple)) and isinstance(new, str):
            try:
                return type(old)(yaml.safe_load(new.replace("(", "[").replace(")", "]")))
            except Exception:
                return new
        return new

    def merge_from_other_cfg(self, other):
        if self.is_frozen():
            raise AttributeError("cannot merge into a frozen CfgNode")
        for k, v in other.items():
            if k == BASE_KEY:
                continue
            if isinstance(v, dict):
                v = v if isinstance(v, CfgNode) else CfgNode(v)
                if isinstance(self.get(k), CfgNode):
                    self[k].merge_from_other_cfg(v)
                else:
                    self[k] = v.clone()
            else:
                self[k] = self._coerce(copy.deepcopy(v), self.get(k))

    @classmethod
    def load_yaml_with_base(cls, filename, allow_unsafe=False):
        """Load a YAML file, resolving `_BASE_` (relative to the file, `~` expanded) depth-first so the
        child overrides its base (config.py:29-70)."""
        with open(filename, "r") as f:
            text = f.read()
        # yacs configs write tuples as python literals, e.g. STEPS: (60000, 80000)
        cfg = yaml.load(text, Loader=_Loader) or {}       # (the safe loader + `!!python/object/apply:eval`, whitelisted)
        if BASE_KEY in cfg:
            base_file = cfg.pop(BASE_KEY)
            if base_file.startswith("~"):
                base_file = os.path.expanduser(base_file)
            if not os.path.isabs(base_file):
                base_file = os.path.join(os.path.dirname(filename), base_file)
            base = cls.load_yaml_with_base(base_file)

            def merge_a_into_b(a, b):
                for k, v in a.items():
                    if isinstance(v, dict) and isinstance(b.get(k), dict):
                        merge_a_into_b(v, b[k])
                    else:
                        b[k] = v
            merge_a_into_b(cfg, base)
            return base
        return cfg

    def merge_from_file(self, cfg_filename, allow_unsafe=True):
        self.merge_from_other_cfg(CfgNode(self.load_yaml_with_base(cfg_filename)))

    def merge_from_list(self, cfg_list):
        assert len(cfg_list) % 2 == 0, "Override list has odd length: {}".format(cfg_list)
        for full_key, v in zip(cfg_list[0::2], cfg_list[1::2]):
            node = self
            parts = full_key.split(".")
            for p in parts[:-1]:
                if p not in node:
                    node[p] = CfgNode()
                node = node[p]
            if isinstance(v, str):
                try:
                    v = yaml.safe_load(v.replace("(", "[").replace(")", "]")) if v[:1] in "([" else yaml.safe_load(v)
                except Exception:
                    pass
            node[parts[-1]] = self._coerce(v, node.get(parts[-1]))


def get_cfg():
    """A fresh copy of the defaults (detectron2/config/config.py:76-86), with the WSL keys added
    (projects/WSL/wsl/config/defaults.py:7-73) since this package exists for that project, and the DeepLab keys
    (projects/DeepLab/deeplab/config.py:5-28), which add to the defaults and change none."""
    from .defaults import _C, add_deeplab_config, add_wsl_config

    cfg = _C.clone()
    add_wsl_config(cfg)
    add_deeplab_config(cfg)
    return cfg
