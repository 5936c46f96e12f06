"""The yardstick of the warper stages behind top-p (min_p, typical_p, epsilon_cutoff, eta_cutoff) and the rule a device row is held to.

Yardstick: HF's own warper classes (transformers generation/logits_process.py) applied to the fp64 copy of the row, their parameter rounded
to fp32 first (the C ABI carries floats).  HF's classes in fp32 are no yardstick: their fp32 cumsum and entropy place the typical and eta cuts
several tokens away in flat tails, while the kernel's sums are exact (64-bit fixed point).

Rule, per stage, comparing the device's row after stages <= s with the yardstick of stage s applied to the device's row after stages < s:
kept entries are bit-equal to the input of the stage; the -inf patterns are equal, except that ONE token may differ, which then must be the
yardstick's kept survivor nearest the cut or its removed token nearest the cut (largest / smallest distance |-log p - H| for typical,
smallest / largest probability for the others).  The caller bounds the share of rows with such a difference (5 %)."""
import torch

STAGES = ("min_p", "typical_p", "epsilon_cutoff", "eta_cutoff")
NO_OP = dict(min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0)


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def hf_warper(stage, value):
    from transformers.generation import logits_process as lp
    cls = dict(min_p=lp.MinPLogitsWarper, typical_p=lp.TypicalLogitsWarper, epsilon_cutoff=lp.EpsilonLogitsWarper, eta_cutoff=lp.EtaLogitsWarper)[stage]
    return cls(f32(value))


def hf64(stage, value, rows):
    """stage's HF class on the fp64 copy of fp32 rows [r, V] (CPU)"""
    return hf_warper(stage, value)(None, rows.double())


def distance64(rows):
    """typical decoding's |-log p - H| in fp64"""
    lsm = torch.log_softmax(rows.double(), dim=-1)
    ent = -(lsm * lsm.exp()).nansum(-1, keepdim=True)
    return (-lsm - ent).abs()


def check_stage(stage, prev, got, ref, where):
    """prev: the stage's input rows (fp32, CPU), got: the device's rows after the stage, ref: hf64 of prev.  Returns the number of rows whose
    -inf pattern differs from the yardstick (each by the one admissible token); asserts everything else."""
    assert got.shape == prev.shape == ref.shape and got.dtype == torch.float32
    kg, kr, kp = torch.isfinite(got), torch.isfinite(ref), torch.isfinite(prev)
    assert not bool((kg & ~kp).any()), (where, "a removed token came back")
    assert torch.equal(got[kg], prev[kg]), (where, "kept entries are not the stage's input bits")
    alive = kp.any(-1)
    assert bool(kg.any(-1)[alive].all()), (where, "a row lost every token")
    differing = 0
    for r in (kg != kr).any(-1).nonzero().flatten().tolist():
        diff = (kg[r] != kr[r]).nonzero().flatten().tolist()
        assert len(diff) == 1, (where, r, "more than one token differs", diff[:8], len(diff))
        j = diff[0]
        x = prev[r].double()
        m = distance64(prev[r:r + 1])[0] if stage == "typical_p" else -x        # the measure that grows away from the kept side
        removed_here = kp[r] & ~kr[r]
        if kr[r, j]:
            assert m[j] == m[kr[r]].max(), (where, r, j, "differs, but is not the yardstick's survivor nearest the cut")
        else:
            assert removed_here[j] and m[j] == m[removed_here].min(), (where, r, j, "differs, but is not the yardstick's removed token nearest the cut")
        differing += 1
    return differing


def ties_whole(prev, got):
    """within equal input values a stage keeps all or none"""
    for r in range(prev.shape[0]):
        v, order = torch.sort(prev[r], stable=True)
        k = torch.isfinite(got[r])[order]
        same = v[1:] == v[:-1]
        if not bool((k[1:][same] == k[:-1][same]).all()):
            return False
    return True
