"""A closest-point certificate in float64 numpy, with no GJK in it (test helper, not product code), and the state
families of the closest-point tests.

Two convex sets A and B are at distance d > 0 with witness points a in A, b in B exactly when, for the unit vector
n = (a - b) / d, a minimises n . x over A and b maximises n . x over B: the plane through either point with normal n
separates the sets, and no pair of points can be closer than the gap between the two planes.  For polytopes both extrema
are attained at vertices, so the check needs the vertices and the face planes only.

A tier-0 record of snk_closest_points (include/snk.h, "The closest points") reports the points on the margin-inflated
surfaces: P = a - n m on A, PB = b + n m on B, distance d - 2 m.  `certificate` undoes the margin and returns the
residuals of
    unit      | |n| - 1 |
    gap       max | P - PB - n dist |
    member_a  how far a = P + n m lies outside core A (0 inside): the prism's face planes, or radius and half length
    member_b  the same for b = PB - n m and core B (the box: |x_i| <= h_i - m, its margin lies inside the nominal box)
    supp_a    | n . a - min over A of n . x |
    supp_b    | n . b - max over B of n . x |
"""
import numpy as np

import np_manifold as nm
import np_model
from conftest import random_state

SHRINK = 0.006          # the second tier's shrink (snk_selfcol.hpp: kShrink)
BOX_FAR = [0.45, 0.3, 0.1]      # beside the snake: pairs within reach, none deep
BOX_NEAR = [0.10, 0.0, 0.1]     # on top of the snake's head: links inside the box, tiers 1 and 2


class Core(object):
    """A core shape in the world: a prism of `sides` sides (0: the implicit cylinder) or a box of half extents `half`."""

    def __init__(self, R, c, sides=None, half=None):
        self.R, self.c, self.sides, self.half = np.asarray(R, float), np.asarray(c, float), sides, half
        if half is not None:
            self.verts = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], float) * half
        elif sides:
            self.verts = nm.hull_vertices(sides)
        else:
            self.verts = None

    def local(self, x):
        return self.R.T @ (np.asarray(x, float) - self.c)

    def outside(self, x):
        """how far the world point x lies outside the shape (0: inside or on it)"""
        l = self.local(x)
        if self.half is not None:
            return max(0.0, float((np.abs(l) - self.half).max()))
        out = abs(l[2]) - nm.CYL_HL
        if self.sides:
            rim = self.verts[0::2, :2]                                # the +z copies, in order round the rim
            for k in range(len(rim)):
                p, q = rim[k], rim[(k + 1) % len(rim)]
                e = q - p
                nrm = np.array([e[1], -e[0]])                         # outward for a rim that runs from +y towards +x
                nrm /= np.linalg.norm(nrm)
                if nrm @ p < 0:
                    nrm = -nrm
                out = max(out, float(nrm @ (l[:2] - p)))
        else:
            out = max(out, float(np.hypot(l[0], l[1]) - nm.CYL_R))
        return max(0.0, out)

    def extreme(self, n, sign):
        """max (sign +1) or min (sign -1) of n . x over the shape"""
        dl = self.R.T @ np.asarray(n, float) * sign
        if self.verts is not None:
            return sign * float((self.verts @ dl).max()) + float(n @ self.c)
        return sign * (nm.CYL_HL * abs(dl[2]) + nm.CYL_R * float(np.hypot(dl[0], dl[1]))) + float(n @ self.c)


def cores(n_modules, state, sides, box=None, margin=0.001):
    """The 2n cylinder cores of a state in link order and, with box = (centre, R, half extents), the box's core."""
    cyl = [Core(R, c, sides=sides) for _, R, _, c in nm.cylinder_frames(n_modules, state)]
    bx = None if box is None else Core(box[1], box[0], half=np.asarray(box[2], float) - margin)
    return cyl, bx


def certificate(A, B, P, PB, n, dist, margin):
    P, PB, n = (np.asarray(x, float) for x in (P, PB, n))
    a, b = P + n * margin, PB - n * margin
    return dict(unit=abs(float(np.linalg.norm(n)) - 1.0), gap=float(np.abs(P - PB - n * dist).max()),
                member_a=A.outside(a), member_b=B.outside(b),
                supp_a=abs(float(n @ a) - A.extreme(n, -1)), supp_b=abs(float(n @ b) - B.extreme(n, +1)))


def surely_tier0(dist, margin):
    """Does the distance alone tell that the record is a tier-0 one?  A record does not say its tier in the oracle, and a
    tier-1 distance is not bounded by -2 margin: its cores overlap, but the shrunk cores' distance can exceed 2 x shrink,
    because a box corner retreats by sqrt(3) x shrink and a cylinder's rim by sqrt(2) x shrink.  So a tier-1 distance is at
    most shrink x (sqrt(3) + sqrt(2)) - 2 (margin + shrink) = 4.9 mm - 2 margin, and anything above 5 mm is tier 0."""
    assert SHRINK * (np.sqrt(3.0) + np.sqrt(2.0)) - 2.0 * (margin + SHRINK) < 5e-3
    return dist > 5e-3


def is_tier2(dist, margin):
    return abs(dist + 2.0 * (margin + SHRINK)) < 1e-9


# ---- the state family of the issue's calibration, and the oracle's lists on it ----
def family(n, k, seed):
    """k random states of the family: flat on the ground at z = 0.03, joint angles up to 0.9 rad, at rest; float32-rounded."""
    rng = np.random.default_rng(seed)
    return np.array([random_state(rng, n, flat=True, z=0.03, qamp=0.9, vamp=0).astype(np.float32).astype(np.float64)
                     for _ in range(k)])


def oracle_overrides(D):
    """The oracle that lists every pair within D (None: its default breaking threshold and room)."""
    if D is None:
        return dict(max_contacts=0, max_self_contacts=4096)
    return dict(breaking_threshold=float(D), relative_breaking_threshold=0, max_self_contacts=4096, max_contacts=0)


def cylinder_of_link(n):
    """{the oracle's link index: cylinder index} (the oracle numbers the tree's links as np_manifold does)"""
    return {i: c for c, (i, _, _, _) in enumerate(nm.cylinder_frames(n, np.concatenate([[0, 0, 0, 0, 0, 0, 1.0],
                                                                                       np.zeros(6 + 2 * n)])))}


def oracle_pairs(e, state, box_state=None):
    """(box rows, link rows) of the oracle env's contacts_full at `state`, each [k, 12] with the link columns (4, 5) turned
    into cylinder indices (box rows: column 5 = 2n), in the oracle's order."""
    n = e.n
    cmap = cylinder_of_link(n)
    e.hard_reset()
    if box_state is not None:
        e.set_box(box_state, np.zeros(29))
    e.set_state(np.asarray(state, float))
    C = e.contacts_full(8192)
    bx = C[C[:, 5] == -2].copy()
    lk = C[C[:, 5] >= 0].copy()
    bx[:, 4] = [cmap[int(i)] for i in bx[:, 4]]
    bx[:, 5] = 2 * n
    lk[:, 4] = [cmap[int(i)] for i in lk[:, 4]]
    lk[:, 5] = [cmap[int(i)] for i in lk[:, 5]]
    return bx, lk


def box_frame(params, box_state=None):
    """(centre, R, half extents) of the obstacle box: the static one of the parameters, or a free box's state"""
    half = np.array(params.obstacle_half[:], float)
    if box_state is None:
        return np.array(params.obstacle_pos[:], float), np.eye(3), half
    return np.asarray(box_state[0:3], float), np_model.quat_to_mat(np.asarray(box_state[3:7], float)), half
