"""numpy restatement of the MLLR branch of asr/adapt/transform.cc ("tr") and asr/train/estimateAdapt.cc ("eA"): the yardstick of the adaptation
tests.

Float / double placement is spelled out: np.float32 where the reference holds a float (postProb cast to `float ck`, `float term`, the products
term * mn_m * mn_n, the accumulator of MLLRTransformer::transform), fp64 for its gsl matrices; sums sequential over the Gaussians in model
order.  Nothing here is taken from the reference's text."""
import struct

import numpy as np

f32 = np.float32
MAX_SV_RATIO = 1.0e-07               # eA:2156
UNSPECIFIED, MLLR = 0, 3


class IndexError_(Exception):
    """jindex_error"""


class KeyError_(Exception):
    """jkey_error"""


class TypeError_(Exception):
    """jtype_error"""


class ParameterError(Exception):
    """jparameter_error"""


class ConsistencyError(Exception):
    """jconsistency_error"""


def is_ancestor(ancestor, child):
    """tr:133-145"""
    if ancestor == 0 or child == 0:
        raise IndexError_("index is zero")
    while child >= ancestor:
        if child == ancestor:
            return True
        child //= 2
    return False


# ---- statistics ------------------------------------------------------------------------------------------------------------------------
def node_gaussians(classes, node):
    """GaussListTrain (eA:68-76): the Gaussians below `node`, in model order"""
    return [g for g, c in enumerate(classes) if is_ancestor(node, int(c))]


def calc_stats(mean, iv, c, sumO, gs, track=False):
    """_calcGi for every row and _calcZ (eA:2101-2153) over the Gaussians `gs` -> G [D][n][n], Z [D][n], ttlFrames (eA:1565-1572), and with
    track the sums of the terms' magnitudes and the number of Gaussians that contributed"""
    mean = np.asarray(mean, f32); iv = np.asarray(iv, f32); D = mean.shape[1]; n = D + 1
    G = np.zeros((D, n, n)); Z = np.zeros((D, n)); aG = np.zeros((D, n, n)); aZ = np.zeros((D, n)); ttl = 0.0; used = 0
    for g in gs:
        ttl += float(c[g])                                                     # double postProb, every Gaussian
        ck = f32(c[g])                                                         # float ck = mix.postProb()
        if ck == 0.0:
            continue
        used += 1
        xi = np.concatenate([mean[g], np.ones(1, f32)])                        # float mn = (n == featLen) ? 1.0 : origMean[n]
        term = ck * iv[g]                                                      # float term = ck * invVar(dim)           [D] float32
        t3 = (term[:, None] * xi[None, :])[:, :, None] * xi[None, None, :]     # term * mn_m * mn_n, float products      [D][n][n]
        assert t3.dtype == f32
        G += t3.astype(np.float64)
        tz = (np.asarray(sumO[g], np.float64) * iv[g].astype(np.float64)).astype(f32)     # float term = sumO(m) * invVar(m): double product
        t2 = tz[:, None] * xi[None, :]                                         # term * mn                               [D][n]
        assert t2.dtype == f32
        Z += t2.astype(np.float64)
        if track:
            aG += np.abs(t3.astype(np.float64)); aZ += np.abs(t2.astype(np.float64))
    iu = np.triu_indices(n)
    for i in range(D):                                                         # only m <= n is accumulated, then copied down (eA:2123-2128)
        U = np.zeros((n, n)); U[iu] = G[i][iu]; G[i] = U + np.triu(U, 1).T
    if track:
        return G, Z, ttl, aG, aZ, used
    return G, Z, ttl


def svd_solve(Gi, zi):
    """eA:2169-2180 -> (w, kept rank)"""
    U, s, Vt = np.linalg.svd(Gi)
    t = U.T @ zi
    with np.errstate(divide="ignore", invalid="ignore"):
        keep = (s / s[0]) >= MAX_SV_RATIO
    t = np.where(keep, t / np.where(keep, s, 1.0), 0.0)
    return Vt.T @ t, int(keep.sum())


def estimate_W(G, Z):
    """MLLREstimatorAdapt::estimate (eA:2158-2186) -> W [D][D + 1]"""
    return np.stack([svd_solve(G[i], Z[i])[0] for i in range(G.shape[0])])


def mix_lhood(W, mean, iv, c, sumO, gs):
    """the auxiliary function: the sum of _calcMixLhood (eA:1603-1620) over the Gaussians `gs` for the transform W"""
    mu = transform_means(W, np.asarray(mean, f32)[gs]); total = 0.0
    for j, g in enumerate(gs):
        ck = f32(c[g])
        if ck == 0.0:
            continue
        for k in range(mu.shape[1]):
            trn = float(mu[j, k])
            total += (float(sumO[g][k]) - 0.5 * float(ck) * trn) * trn * float(iv[g][k])
    return total


# ---- the parameter tree ----------------------------------------------------------------------------------------------------------------
class Param(object):
    """MLLRParam (tr:556-650)"""

    def __init__(self, regClass=0, size=0, matrix=None, bias=None):
        self.regClass, self.size = regClass, size
        self.matrix = np.zeros((size, size)) if matrix is None else np.array(matrix, np.float64)
        self.bias = np.zeros(0) if bias is None else np.array(bias, np.float64)

    def copy(self):
        return Param(self.regClass, self.size, self.matrix.copy(), self.bias.copy())

    def assign(self, W):
        """operator=(const gsl_matrix*) tr:622-650"""
        W = np.asarray(W, np.float64); D = W.shape[0]; assert W.shape == (D, D + 1)
        self.size = D; self.matrix = W[:, :D].copy(); self.bias = W[:, D].copy()

    def W(self):
        return np.concatenate([self.matrix, self.bias[:, None]], axis=1)

    def text(self):
        """ParamBase::write (tr:365-372) with MLLRParam::_putParams (tr:576-587)"""
        s = "<AdaptType> MLLR\n<RegClass> %d\n<MLLRParam> %d\n" % (1 if self.regClass == 0 else self.regClass, self.size)
        for m in range(self.size):
            s += "".join(" %g" % v for v in self.matrix[m]) + "\n"
        if len(self.bias):
            s += "<BiasOffset> %d\n" % len(self.bias) + "".join(" %g" % v for v in self.bias) + "\n"
        return s + "<EndClass>\n"


class ParamTree(object):
    """ParamTree (tr:789-950) of MLLR parameters"""

    def __init__(self, text=None):
        self.map, self.type = {}, UNSPECIFIED
        if text:
            self.read(text)

    def clear(self):
        self.map, self.type = {}, UNSPECIFIED

    def hasIndex(self, rc):
        return rc in self.map

    def _nearest(self, rc, useAncestor, mllr):
        if mllr:
            self.type = MLLR
        if rc == 0:
            raise IndexError_("Regression class index is zero")
        if rc in self.map:
            return self.map[rc]
        if not useAncestor:
            raise IndexError_("No parameters for index %d." % rc)
        reg = rc // 2
        while reg > 0 and reg not in self.map:
            reg //= 2
        if reg == 0 and not mllr:
            raise IndexError_("No ancestor for node %d." % rc)
        par = Param() if reg == 0 else self.map[reg].copy()
        par.regClass = rc; self.map[rc] = par
        return par

    def find(self, rc, useAncestor=True):
        """tr:835-860"""
        return self._nearest(rc, useAncestor, False)

    def findMLLR(self, rc, useAncestor=True):
        """tr:898-925"""
        return self._nearest(rc, useAncestor, True)

    def text(self):
        """tr:824-833: the map in index order"""
        return "".join(self.map[k].text() for k in sorted(self.map))

    def read(self, text):
        """tr:927-950 with ParamBase::param / _readParams (tr:339-407): tokens are <Symbol> and numbers separated by white space"""
        self.clear()
        tok = text.replace("<", " <").replace(">", "> ").split(); p = 0
        new = {}
        if text and not tok:
            raise TypeError_("Unable to determine adaptation type.")
        while p < len(tok):
            if tok[p] != "<AdaptType>":
                raise TypeError_("Unable to determine adaptation type.")
            if tok[p + 1] != "MLLR":
                raise TypeError_("Unknown adaptation type.")
            p += 2; par = Param()
            while tok[p] != "<EndClass>":
                sym = tok[p]; p += 1
                if sym == "<AdaptType>":
                    if tok[p] != "MLLR":
                        raise ParameterError("Attempted to read parameters of wrong type.")
                    p += 1
                elif sym == "<RegClass>":
                    par.regClass = int(tok[p]); p += 1
                elif sym in ("<RAPTParam>", "<SLAPTParam>"):
                    raise ParameterError("Attempted to read MLLR parameters.")
                elif sym == "<MLLRParam>":
                    n = int(tok[p]); p += 1
                    par.size = n; par.matrix = np.array([float(t) for t in tok[p:p + n * n]]).reshape(n, n); p += n * n
                elif sym == "<BiasOffset>":
                    n = int(tok[p]); p += 1
                    par.bias = np.array([float(t) for t in tok[p:p + n]]); p += n
                else:
                    raise ParameterError("Unexpected symbol %s in conformal parameter file." % sym)
            p += 1
            new.setdefault(par.regClass, par)
        if not new:
            raise ConsistencyError("Unable to determine adaptation type.")
        self.map, self.type = new, MLLR


# ---- estimation over the tree ----------------------------------------------------------------------------------------------------------
def tree_nodes(classes):
    """EstimatorTreeMLLR (eA:3143-3165): the classes are the leaves, their ancestors the internal nodes -> (leaves, nodes), ascending"""
    leaves = sorted(set(int(c) for c in classes))
    if leaves and leaves[0] == 0:
        raise IndexError_("Regression class index must be >= 1")
    nodes = set()
    for l in leaves:
        while l > 0:
            nodes.add(l); l //= 2
    return leaves, sorted(nodes)


def estimate_tree(classes, ttl, solve, threshold, speaker=0):
    """estimateAdaptationParameters (eA:3064-3078) with LeafIterator::estimate (eA:3105-3133).  ttl: {node: ttlFrames}; solve(node) -> W.
    -> (ParamTree, plan rows (speaker, node, leaf, copy))"""
    leaves, _ = tree_nodes(classes)
    tree = ParamTree(); plan = []
    thr = float(f32(threshold))                                                # static float EstimateThreshold
    for leaf in leaves:
        rc = leaf
        while rc > 0:
            if ttl[rc] > thr:
                break
            rc //= 2
        if rc == 0:
            rc = 1
        if leaf != rc and tree.type == MLLR and tree.hasIndex(rc):
            tree.find(leaf, True); plan.append((speaker, rc, leaf, 1)); continue
        W = solve(rc)
        tree.findMLLR(leaf).assign(W); tree.findMLLR(rc).assign(W)             # eA:2188-2192
        plan.append((speaker, rc, leaf, 0))
    return tree, plan


# ---- applying the transforms -----------------------------------------------------------------------------------------------------------
def transform_means(W, mu):
    """MLLRTransformer::transform (tr:1770-1785) for rows of means [N][D]: float comp = bias; comp += A[m][n] * from[n] (a double sum rounded to
    float after every term)"""
    W = np.asarray(W, np.float64); mu = np.asarray(mu, f32); D = W.shape[0]
    comp = np.broadcast_to(W[:, D].astype(f32), mu.shape).copy()
    for n in range(D):
        comp = (comp.astype(np.float64) + W[None, :, n] * mu[:, n, None].astype(np.float64)).astype(f32)
    return comp


def tree_node(tree, rc):
    """BaseTree::node(idx, useAncestor = true) (tr:2030-2049) over the classes of the parameter tree"""
    if rc == 0:
        raise IndexError_("Regression class index must be >= 1")
    idx = rc
    if tree.hasIndex(idx):
        return idx
    while idx > 1:
        idx //= 2
        if tree.hasIndex(idx):
            return idx
    raise KeyError_("Could not find node %d." % idx)


def transform_tree(tree, classes, mean):
    """TransformerTree::transform (tr:2149-2163) -> the new means"""
    mean = np.asarray(mean, f32); out = np.empty_like(mean)
    where = np.array([tree_node(tree, int(c)) for c in classes])
    for node in sorted(set(where)):
        sel = where == node
        out[sel] = transform_means(tree.map[node].W(), mean[sel])
    return out


# ---- codebook and distribution files with the regression-class table (codebookBasic.cc:258-309, 352-405, 962-983) -------------------------
def _wstr(b):
    return struct.pack(">h", len(b)) + b + b"\0"


def codebook_file(m, classes=None):
    """the set file of a tests.train_np.Model; classes: per Gaussian a class or a list of classes, None for a file without the table"""
    out = struct.pack(">iii", 64207531, 0, m.K)
    for k in range(m.K):
        out += _wstr(m.cbNames[k].encode()) + struct.pack(">iiiiiii", m.refN[k], m.D, m.D, 1, 2, 0 if classes is None else 1, 0)
        for g in range(m.off[k], m.off[k + 1]):
            out += struct.pack(">f", m.count[g]) + m.mean[g].astype(">f4").tobytes() + m.cv[g].astype(">f4").tobytes() + struct.pack(">f", m.det[g])
        if classes is not None:
            for g in range(m.off[k], m.off[k + 1]):
                cl = classes[g] if isinstance(classes[g], (list, tuple)) else [classes[g]]
                out += struct.pack(">h", len(cl)) + b"".join(struct.pack(">H", int(c)) for c in cl)
        out += struct.pack(">i", 123456789)
    return out


def distrib_file(m):
    out = struct.pack(">i", m.K)
    for k in range(m.K):
        out += _wstr(m.dsNames[k].encode()) + _wstr(m.cbNames[k].encode()) + struct.pack(">if", -m.refN[k], 0.0)
        out += m.val[m.off[k]:m.off[k + 1]].astype(">f4").tobytes()
    return out
