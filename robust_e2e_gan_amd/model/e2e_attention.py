"""Attention modules (mirror of model/e2e_attention.py): AttLoc (:199-299), AttDot (:63-121), AttAdd (:124-196), AttCov (:302-389)
and AttCovLoc (:602-698).

The reference evaluates an attention's forward once per decoder step as ~10 small ATen ops; here the whole step is fused HIP
(csrc/attloc.hip for ``location`` and ``coverage_location``, csrc/attstep.hip for ``dot``, ``add`` and ``coverage``) driven from the
decoder loop (ops.DecoderLoopFn) and from the beam search, so the modules only hold the parameters, under the reference's names and
shapes, and say which step they are (``kind``).  The coverage types carry cov_{i+1} = cov_i + w_i with cov_0 the uniform row, the sum of
the reference's ``att_prev_list``.  The other seven attention classes of the reference (noatt, location2d, location_recurrent and the
four multi-head types) and non-softmax ``aact_fuc`` are out of scope and refused by E2E."""
import torch

from .e2e_common import ConvParams, LinearParams


class AttLoc(torch.nn.Module):
    kind = 'location'

    def __init__(self, eprojs, dunits, att_dim, aconv_chans, aconv_filts, aact_fuc='softmax'):
        super(AttLoc, self).__init__()
        if aact_fuc != 'softmax':
            raise NotImplementedError('only the softmax attention activation is on the hot path')
        self.mlp_enc = LinearParams(eprojs, att_dim)
        self.mlp_dec = LinearParams(dunits, att_dim, bias=False)
        self.mlp_att = LinearParams(aconv_chans, att_dim, bias=False)
        self.loc_conv = ConvParams(1, aconv_chans, 1, 2 * aconv_filts + 1, bias=False, padding=(0, aconv_filts))
        self.gvec = LinearParams(att_dim, 1)
        self.dunits, self.eprojs, self.att_dim = dunits, eprojs, att_dim
        self.aconv_chans, self.aconv_filts = aconv_chans, aconv_filts

    def reset(self):
        """The reference caches pre_compute_enc_h between steps; the fused loop owns that state."""
        return None


class AttDot(torch.nn.Module):
    """e = sum_a tanh(mlp_enc(h))[t,a] * tanh(mlp_dec(z))[a]; the only type whose mlp_dec has a bias."""
    kind = 'dot'

    def __init__(self, eprojs, dunits, att_dim):
        super(AttDot, self).__init__()
        self.mlp_enc = LinearParams(eprojs, att_dim)
        self.mlp_dec = LinearParams(dunits, att_dim)
        self.dunits, self.eprojs, self.att_dim = dunits, eprojs, att_dim

    def reset(self):
        return None


class AttAdd(torch.nn.Module):
    """e = gvec . tanh(mlp_enc(h)[t] + mlp_dec(z)) + gvec_b"""
    kind = 'add'

    def __init__(self, eprojs, dunits, att_dim):
        super(AttAdd, self).__init__()
        self.mlp_enc = LinearParams(eprojs, att_dim)
        self.mlp_dec = LinearParams(dunits, att_dim, bias=False)
        self.gvec = LinearParams(att_dim, 1)
        self.dunits, self.eprojs, self.att_dim = dunits, eprojs, att_dim

    def reset(self):
        return None


class AttCov(torch.nn.Module):
    """AttAdd with wvec(cov[t]) inside the tanh; wvec is a Linear(1, att_dim): weight (att_dim, 1), bias (att_dim)."""
    kind = 'coverage'

    def __init__(self, eprojs, dunits, att_dim):
        super(AttCov, self).__init__()
        self.mlp_enc = LinearParams(eprojs, att_dim)
        self.mlp_dec = LinearParams(dunits, att_dim, bias=False)
        self.wvec = LinearParams(1, att_dim)
        self.gvec = LinearParams(att_dim, 1)
        self.dunits, self.eprojs, self.att_dim = dunits, eprojs, att_dim

    def reset(self):
        return None


class AttCovLoc(torch.nn.Module):
    """AttLoc's parameters and energy, the location conv reading cov instead of the previous attention weights."""
    kind = 'coverage_location'

    def __init__(self, eprojs, dunits, att_dim, aconv_chans, aconv_filts):
        super(AttCovLoc, self).__init__()
        self.mlp_enc = LinearParams(eprojs, att_dim)
        self.mlp_dec = LinearParams(dunits, att_dim, bias=False)
        self.mlp_att = LinearParams(aconv_chans, att_dim, bias=False)
        self.loc_conv = ConvParams(1, aconv_chans, 1, 2 * aconv_filts + 1, bias=False, padding=(0, aconv_filts))
        self.gvec = LinearParams(att_dim, 1)
        self.dunits, self.eprojs, self.att_dim = dunits, eprojs, att_dim
        self.aconv_chans, self.aconv_filts = aconv_chans, aconv_filts

    def reset(self):
        return None
