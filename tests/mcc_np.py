"""numpy restatement of btk/localization's multichannel cross-correlation localiser (MCCLocalizer.h:55-301, MCCLocalizer.cc:10-576, the delay
functions of localization.cc:110-142), written from the behaviour DESIGN 4.4l lists: the two far-field grid builders with the reference's
float arithmetic (np.float32 where it uses float), calcCovarianceMatrix, the cost from the eigenvalues with the reference's sign and zero
handling, the N-best insertion and MCCCalculator.  Deviations shared with the product: setPositionsOfMicrophones copies every row and
measures from microphone 0; the circular walk takes |sin|, |cos| in its polar step and ends when the azimuth reaches 2 pi."""
import numpy as np

f32 = np.float32
SSPEED = 343740.0
TPI = 6.28318530717958647692
PI_2, PI_4, PI = np.pi / 2, np.pi / 4, np.pi


# sinf, cosf, asinf, acosf: the double function rounded to float, which is what a correctly rounded libm returns
def sinf(x): return f32(np.sin(np.float64(x)))
def cosf(x): return f32(np.cos(np.float64(x)))
def asinf(x): return f32(np.arcsin(np.float64(x)))
def acosf(x): return f32(np.arccos(np.float64(x)))


class Grid(object):
    def __init__(self, kind, nChan, fs=16000):
        self.kind, self.C, self.fs = kind, int(nChan), int(fs)
        self.mpos = np.zeros((self.C, 3)); self.hypo = np.zeros(3); self.maxTimeDelay = f32(-1); self.constV = f32(0)

    # ---- geometry
    def setDistanceBtwMicrophones(self, distance):
        d = f32(distance); n1 = f32(self.C - 1)
        for m in range(self.C):
            self.mpos[m] = (0.0, float(f32(m) * d), 0.0)
        self.constV = f32(0.99 * SSPEED / float(n1 * d * f32(self.fs)))
        self.maxTimeDelay = f32(float(n1 * d) / SSPEED)

    def setPositionsOfMicrophones(self, mpos):
        mpos = np.asarray(mpos, np.float64); self.mpos[:] = mpos
        p0 = mpos[0].astype(f32); maxDist = f32(-1)
        for m in range(1, self.C):
            dx, dy, dz = p0 - mpos[m].astype(f32)
            dist = np.sqrt(f32(f32(dx * dx + dy * dy) + dz * dz))
            if dist > maxDist:
                maxDist = dist
        self.constV = f32(0.99 * SSPEED / float(maxDist * f32(self.fs)))
        self.maxTimeDelay = f32(float(maxDist) / SSPEED)

    def setRadius(self, radius, height=0.0):
        r = f32(radius); bias = f32(TPI / float(f32(self.C)))
        for m in range(self.C):
            a = f32(m) * bias
            self.mpos[m] = (float(r * cosf(a)), float(r * sinf(a)), float(f32(height)))
        self.constV = f32(SSPEED / float(f32(2) * r * f32(self.fs)))
        self.maxTimeDelay = f32(float(f32(2) * r) / SSPEED)

    def D(self):
        return int(f32(self.fs) * self.maxTimeDelay)

    # ---- the walk
    def reset(self):
        self.hypo[:] = 0.0

    def nextSearchGrid(self):
        cv = self.constV
        if self.kind == "linear":
            az = f32(self.hypo[1]); oldSin = sinf(az)
            if float(az) < PI_2:
                newSin = f32(oldSin + cv)
                newAz = f32(PI_2) if newSin >= 1 else asinf(newSin)
            elif float(az) < 3 * PI_2:
                newAz = f32(3 * PI_2)
            else:
                newSin = f32(oldSin + cv)
                if float(newSin) + float(cv) / 2.0 >= 0:
                    return False
                newAz = f32(TPI + float(asinf(newSin)))
            self.hypo[1] = float(newAz)
            return True
        az = f32(self.hypo[1]); pol = f32(self.hypo[2])
        if float(az) >= TPI:
            return False
        a = float(az)
        if (PI_4 <= a < 3 * PI_4) or (5 * PI_4 <= a < 7 * PI_4):
            val1 = f32(cv / np.abs(sinf(az)))
        else:
            val1 = f32(cv / np.abs(cosf(az)))
        newPol = asinf(val1) if val1 < 1 else f32(PI_2)
        if float(f32(newPol + pol)) < PI:
            newPol = f32(newPol + pol); newAz = az
        else:
            val2 = f32(cv / sinf(newPol))
            newAz = f32(np.arccos(float(f32(cv / val2)))) if val2 < 1 else f32(PI)
            newAz = f32(newAz + az)
        if float(newAz) >= TPI:
            return False
        self.hypo[1] = float(newAz); self.hypo[2] = float(newPol)
        return True

    def getTimeDelays(self):
        d = np.zeros(self.C)
        if self.kind == "linear":
            az = f32(self.hypo[1])
            for i in range(1, self.C):
                dist = f32(abs(self.mpos[i, 1] - self.mpos[0, 1]))
                d[i] = -float(dist) * np.sin(float(az)) / SSPEED
            return d
        az = f32(self.hypo[1]); pol = f32(self.hypo[2])
        cx = f32(-sinf(pol) * cosf(az)); cy = f32(-sinf(pol) * sinf(az)); cz = f32(-cosf(pol))
        for i in range(self.C):
            d[i] = float(f32((float(cx) * self.mpos[i, 0] + float(cy) * self.mpos[i, 1] + float(cz) * self.mpos[i, 2]) / SSPEED))
        return d

    def enumerate(self, cap=65536):
        """-> positions [G][3], delays [G][C], tau [G][C]"""
        keep = self.hypo.copy(); self.reset(); pos, dl = [], []
        while True:
            assert len(pos) < cap, "the walk does not end"
            pos.append(self.hypo.copy()); dl.append(self.getTimeDelays())
            if not self.nextSearchGrid():
                break
        self.hypo[:] = keep
        dl = np.array(dl)
        return np.array(pos), dl, tau_of(self.fs, dl)


def tau_of(fs, delays):
    """(int)(float)(fs * delay), truncation toward zero"""
    return np.trunc((float(fs) * np.asarray(delays, np.float64)).astype(f32)).astype(np.int32)


def covariance(block, tau, D):
    """calcCovarianceMatrix: block [C][L] float32, tau [C] -> R [C][C], lower triangle only (dsyr Lower), the upper zero"""
    block = np.asarray(block, f32); Cn, L = block.shape
    if L < 2 * D:
        raise ValueError("Data samples are insufficient")
    n = np.arange(L - D)
    X = np.stack([block[c, (n + int(tau[c])) % L] for c in range(Cn)]).astype(np.float64)     # a negative index reads the block's own tail
    return np.tril(X @ X.T) * (1.0 / (L - D))


def eigenvalues(R):
    """the eigenvalues of the symmetric matrix the lower triangle stands for"""
    return np.linalg.eigvalsh(np.tril(R) + np.tril(R, -1).T)


def cost_of(R, normalizeVariance=True):
    """calcObjectiveFunction: negative eigenvalues negated, an exactly zero one gives 0.0, else sum log lambda - sum log R_ii
    -> (cost, the eigenvalues as the reference leaves them)"""
    ev = eigenvalues(R).copy(); ldet = lnrm = 0.0
    for i in range(ev.size):
        if ev[i] < 0:
            ev[i] = -ev[i]
        elif ev[i] <= 0:
            return 0.0, ev
        ldet += np.log(ev[i]); lnrm += np.log(R[i, i])
    return ldet - (lnrm if normalizeVariance else 0.0), ev


def nbest(costs, maxSource):
    """the insertion of MCCLocalizer::search (strict `<`, grid order) -> [(cost, grid index)] of maxSource entries, index -1 = never filled"""
    lst = [(100000.0, -1)] * maxSource
    for g, c in enumerate(costs):
        if c < lst[-1][0]:
            for i in range(maxSource):
                if c < lst[i][0]:
                    lst = lst[:i] + [(c, g)] + lst[i:-1]
                    break
    return lst


def localize(block, tauTab, D, maxSource=1):
    """one next() of MCCLocalizer -> dict(costs [G], kappa [G], best [(cost, g)], eig {g: eigenvalues}, Rlast)"""
    G = tauTab.shape[0]; costs = np.zeros(G); kappa = np.zeros(G); evs = []
    for g in range(G):
        R = covariance(block, tauTab[g], D)
        costs[g], ev = cost_of(R)
        evs.append(np.sort(np.abs(ev))); kappa[g] = np.inf if evs[-1][0] <= 0 else evs[-1][-1] / evs[-1][0]
    best = nbest(costs, maxSource)
    return dict(costs=costs, kappa=kappa, best=best, eig={g: evs[g] for _, g in best if g >= 0}, Rlast=R)


def calculate(block, delays, fs, D, normalizeVariance=True):
    """one next() of MCCCalculator -> (cost, tau, R, eigenvalues)"""
    tau = tau_of(fs, delays); R = covariance(block, tau, D); c, ev = cost_of(R, normalizeVariance)
    return c, tau, R, np.sort(np.abs(ev))
