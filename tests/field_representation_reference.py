"""The reference of the representation execute (fmmbem_plan_execute_representation), composed on the CPU with no product code in it.

phi = S[sigma] - D[mu] and its gradient at the points of a case of tests/field_gradient_reference.py, the points' own flags
ignored: every point takes the single layer as a flag-0 target and the double layer as a flag-1 target.  So the reference is two
references, one per layer, each over the SAME points with the flags set all 0 / all 1:

  values      oracle.TargetOracle(v, pts, all f).matvec -- the oracle's own FMM over separate targets
  gradients   field_gradient_reference.Reference's composition (gamma in numpy over the listed near pairs; P2M, M2M, M2L, L2L by the
              oracle's operators; the long-double gradient of L), built on the layer's flags

LayerReference is Reference with the flags of the case replaced; parts(name, p) returns the two layers' values and gradients for
the case's two vectors (x: the density sigma, x2: the surface potential mu -- independent seeds)."""
import numpy as np

import field_gradient_reference as G
from oracle import oracle as O


class LayerReference(G.Reference):
    """G.Reference on a case's panels and points with EVERY flag set to `flag`"""

    def __init__(self, name, flag):
        c = dict(G.make_case(name))
        c["flags"] = np.full(len(c["pts"]), flag, dtype=np.uint8)
        self.name, self.c = name, c
        self.v, self.pts, self.flags = c["v"], c["pts"], c["flags"]
        self.T = O.TargetOracle(self.v, self.pts, self.flags, K=G.K, theta=G.THETA, ncrit=c["ncrit"])
        self.info = self.T.info()
        self.g = G.geometry(self.v)
        self.sb, self.tb = self.T.boxes("source"), self.T.boxes("target")
        self.perm = self.T.perm().astype(np.int64)
        tree, given = self.T.target_perm()
        self.tree, self.given = tree.astype(np.int64), given.astype(np.int64)
        self.P, self.F = self.T.target_points()
        self.near = {}
        for s_, t_ in self.T.pairs("p2p"):
            self.near.setdefault(int(t_), []).append(int(s_))
        base = G.reference(name)                           # the case's vectors: x the density, x2 the surface potential
        self.x, self.x2 = base.x, base.x2
        self._near, self._far, self._limit = {}, {}, {}


_LAYERS = {}
_PARTS = {}


def layer(name, flag):
    if (name, flag) not in _LAYERS:
        _LAYERS[(name, flag)] = LayerReference(name, flag)
    return _LAYERS[(name, flag)]


def parts(name, p):
    """dict(S, D (given targets,), gS, gD (given targets, 3)): the single layer of x and the double layer of x2 at order p, each as
    its own execute / execute_gradient would return it; the representation is S - D and gS - gD"""
    if (name, p) not in _PARTS:
        r0, r1 = layer(name, 0), layer(name, 1)
        _PARTS[(name, p)] = dict(S=r0.T.matvec(r0.x, p), D=r1.T.matvec(r1.x2, p), gS=r0.gradient(p, "x"), gD=r1.gradient(p, "x2"))
    return _PARTS[(name, p)]
