"""The callers of the hot path, restated for the build's own driver: the E2PN
backbone wiring (experiments/se3ete.3dmatch/backbone.py:8-78, 5-stage variant experiments/se3eti.kitti/backbone.py),
the SE3ET forward (experiments/se3ete.3dmatch/model.py:20-227) and the per-variant configuration values
(experiments/<variant>/config.py).  Module and parameter names equal the reference's, so a reference checkpoint loads
with load_state_dict(strict=True)."""
from types import SimpleNamespace

import threading

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import functional as SF
from . import tables
from .modules.e2pn import InvOutBlockEPN, LiftBlockEPN, ResnetBottleneckBlockEPN, SimpleBlockEPN
from .modules.geotransformer import GeometricTransformer, LocalGlobalRegistration, SuperPointMatching
from .modules.kpconv import LastUnaryBlock, UnaryBlock, nearest_upsample
from .modules.ops import index_select, point_to_node_partition
from .modules.sinkhorn import LearnableLogOptimalTransport

_BLOCKS_E = ['self_eq', 'cross_a_soft', 'self_eq', 'cross_r_soft', 'self', 'cross', 'self', 'cross', 'self', 'cross']
_BLOCKS_I = ['self_eq', 'cross', 'self_eq', 'cross', 'self_eq', 'cross']

VARIANTS = {
    #            init_dim out  gn  gt_in hidden gt_out blocks   n_eq stages voxel  base_radius
    'se3ete':   (64, 256, 32, 1024, 256, 256, _BLOCKS_E, 2, 4, 0.025, 2.5),
    'se3eti':   (64, 256, 32, 1024, 256, 256, _BLOCKS_I, 0, 4, 0.025, 2.5),
    'se3ete2':  (32, 128, 16, 512, 128, 128, _BLOCKS_E, 2, 4, 0.025, 2.5),
    'se3eti2':  (32, 128, 16, 512, 128, 128, _BLOCKS_I, 0, 4, 0.025, 2.5),
    'se3eti_kitti': (64, 256, 32, 2048, 128, 256, _BLOCKS_I, 0, 5, 0.3, 4.25),
    'micro_e':  (8, 32, 4, 128, 32, 32, _BLOCKS_E, 2, 4, 0.025, 2.5),
    'micro_i':  (8, 32, 4, 128, 32, 32, _BLOCKS_I, 0, 4, 0.025, 2.5),
}


def make_cfg(variant='se3ete', attention_dtype='float32'):
    """attention_dtype (not a reference key): 'float32' = the reference's arithmetic; 'bfloat16' stores the geometric embedding
    of the RPE self-attention layers in bf16 (BASELINE.json configs[2], 'bf16 attention')."""
    init_dim, out_dim, gn, gt_in, hidden, gt_out, blocks, n_eq, stages, voxel, base_radius = VARIANTS[variant]
    ns = SimpleNamespace
    kitti = variant.endswith('kitti')
    cfg = ns(variant=variant)
    cfg.backbone = ns(num_stages=stages, init_voxel_size=voxel, kernel_size=15, base_radius=base_radius, base_sigma=2.0,
                      init_radius=base_radius * voxel, init_sigma=2.0 * voxel, group_norm=gn, input_dim=1,
                      init_dim=init_dim, output_dim=out_dim)
    cfg.epn = ns(kanchor=6, quotient_factor=4, num_kernel_points=15, non_sep_conv=True, equiv_mode_kp=True,
                 fixed_kernel_points='center', rot_by_permute=True, ignore_steer_constraint=False, epn_kernel=False,
                 att_pooling=False, att_permute=False, dual_feature=False, gather_by_idxing=False, use_batch_norm=True,
                 batch_norm_momentum=0.99, KP_influence='linear', aggregation_mode='sum')
    cfg.model = ns(ground_truth_matching_radius=0.6 if kitti else 0.05, num_points_in_patch=128 if kitti else 64,
                   num_sinkhorn_iterations=100)
    cfg.coarse_matching = ns(num_targets=128, overlap_threshold=0.1, num_correspondences=256, dual_normalization=True)
    cfg.geotransformer = ns(input_dim=gt_in, hidden_dim=hidden, output_dim=gt_out, num_heads=4, blocks=list(blocks),
                            sigma_d=4.8 if kitti else 0.2, sigma_a=15, angle_k=3, supervise_rotation=False,
                            reduction_a='max', align_mode='0', alternative_impl=False, n_level_equiv=n_eq,
                            attention_dtype=attention_dtype)
    cfg.fine_matching = ns(topk=2 if kitti else 3, acceptance_radius=0.6 if kitti else 0.1, mutual=True,
                           confidence_threshold=0.05, use_dustbin=False, use_global_score=False,
                           correspondence_threshold=3, correspondence_limit=None, num_refinement_steps=5)
    # training (experiments/<variant>/config.py: coarse_loss, fine_loss, loss, optim)
    cfg.coarse_loss = ns(positive_margin=0.1, negative_margin=1.4, positive_optimal=0.1, negative_optimal=1.4, log_scale=40 if kitti else 24,
                         positive_overlap=0.1)
    cfg.fine_loss = ns(positive_radius=0.6 if kitti else 0.05)
    cfg.loss = ns(weight_coarse_loss=1.0, weight_fine_loss=1.0)
    cfg.optim = ns(lr=1e-4, lr_decay=0.95, lr_decay_steps=4 if kitti else 1, weight_decay=1e-6, max_epoch=160 if kitti else 40, grad_acc_steps=1)
    cfg.neighbor_limits = [38, 36, 36, 38, 38][:stages]
    # evaluation (experiments/se3ete.3dmatch/config.py:54-59, experiments/se3eti.kitti/config.py:58-62; se3et_amd.evaluation)
    cfg.eval = ns(acceptance_overlap=0.0, acceptance_radius=1.0 if kitti else 0.1, inlier_ratio_threshold=0.05,
                  rre_threshold=5.0 if kitti else 15.0, rte_threshold=2.0 if kitti else 0.3)
    if not kitti:
        cfg.eval.rmse_threshold = 0.2
    # eval.py --method ransac (experiments/se3ete.3dmatch/config.py:62-65, experiments/se3eti.kitti/config.py:65-68; se3et_amd.ransac)
    cfg.ransac = ns(distance_threshold=0.3 if kitti else 0.05, num_points=4 if kitti else 3, num_iterations=50000)
    return cfg


class E2PN(nn.Module):
    """Encoder: lift, (simple, resnet) at stage 1, then per stage (strided resnet, resnet, resnet) with radius/sigma
    doubling; decoder: nearest upsample + unary blocks down to stage 2.  Returns [fine inv feats, ..., coarse eq feats]."""

    def __init__(self, input_dim, output_dim, init_dim, init_radius, init_sigma, group_norm, config_epn, num_stages=4):
        super().__init__()
        self.num_stages = num_stages
        R = ResnetBottleneckBlockEPN
        self.preprocess = LiftBlockEPN('lift_epn', input_dim, config_epn)
        self.encoder1_1 = SimpleBlockEPN('simple', input_dim, init_dim, init_radius, init_sigma, group_norm, config_epn)
        self.encoder1_2 = R('resnetb', init_dim, init_dim * 2, init_radius, init_sigma, group_norm, config_epn)
        dim, radius, sigma = init_dim * 2, init_radius, init_sigma
        for s in range(2, num_stages + 1):
            setattr(self, 'encoder%d_1' % s, R('resnetb_strided', dim, dim, radius, sigma, group_norm, config_epn))
            radius, sigma = radius * 2, sigma * 2
            setattr(self, 'encoder%d_2' % s, R('resnetb', dim, dim * 2, radius, sigma, group_norm, config_epn))
            setattr(self, 'encoder%d_3' % s, R('resnetb' if s < num_stages else 'resnetb_epn', dim * 2, dim * 2, radius,
                                               sigma, group_norm, config_epn))
            setattr(self, 'equ2inv%d' % s, InvOutBlockEPN('inv_epn', dim * 2, config_epn))
            dim *= 2
        # dim == init_dim * 2^(S-1) is the width of the last stage
        for s in range(num_stages - 1, 2, -1):       # stage s is init_dim * 2^s wide; input = upsampled stage s+1 + stage s
            setattr(self, 'decoder%d' % s, UnaryBlock(init_dim * 2 ** s * 3, init_dim * 2 ** s, group_norm))
        self.decoder2 = LastUnaryBlock(init_dim * 4 * 3, output_dim)
        self.equ2inv = InvOutBlockEPN('inv_epn', output_dim, config_epn)

    def forward(self, feats, data_dict):
        pts, nb = data_dict['points'], data_dict['neighbors']
        sub, up = data_dict['subsampling'], data_dict['upsampling']
        at_stage = SF.norm_segments.at_stage          # per-pair GroupNorm statistics of a stacked batch need the stage a block runs at
        at_stage(0)
        x = self.preprocess(feats)
        x = self.encoder1_1(x, pts[0], pts[0], nb[0])
        x = self.encoder1_2(x, pts[0], pts[0], nb[0])
        inv = {}
        for s in range(2, self.num_stages + 1):
            at_stage(s - 1, support=s - 2)
            x = getattr(self, 'encoder%d_1' % s)(x, pts[s - 1], pts[s - 2], sub[s - 2])
            at_stage(s - 1)
            x = getattr(self, 'encoder%d_2' % s)(x, pts[s - 1], pts[s - 1], nb[s - 1])
            x = getattr(self, 'encoder%d_3' % s)(x, pts[s - 1], pts[s - 1], nb[s - 1])
            inv[s] = getattr(self, 'equ2inv%d' % s)(x)
        feats_list = [x]
        latent = inv[self.num_stages]
        for s in range(self.num_stages - 1, 1, -1):
            at_stage(s - 1)
            dec = getattr(self, 'decoder%d' % s)
            if SF.AG.needs_grad(latent, inv[s], dec.mlp.weight):
                latent = dec(torch.cat((nearest_upsample(latent, up[s - 1]), inv[s]), 1))
            else:                     # inference: the dense layer's coarse half runs before the upsampling, nothing is concatenated
                latent = dec.forward_upsampled(latent, up[s - 1], inv[s])
            feats_list.append(latent)
        at_stage(None)
        feats_list.reverse()
        return feats_list


class SE3ET(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        self.num_points_in_patch = cfg.model.num_points_in_patch
        b, g = cfg.backbone, cfg.geotransformer
        self.backbone = E2PN(b.input_dim, b.output_dim, b.init_dim, b.init_radius, b.init_sigma, b.group_norm, cfg.epn,
                             num_stages=b.num_stages)
        self.transformer = GeometricTransformer(g.input_dim, g.output_dim, g.hidden_dim, g.num_heads, g.blocks, g.sigma_d,
                                                g.sigma_a, g.angle_k, supervise_rotation=g.supervise_rotation,
                                                reduction_a=g.reduction_a, na=cfg.epn.kanchor, align_mode=g.align_mode,
                                                alternative_impl=g.alternative_impl, n_level_equiv=g.n_level_equiv)
        self.transformer.embedding.embedding_dtype = {'float32': torch.float32, 'bfloat16': torch.bfloat16}[
            getattr(g, 'attention_dtype', 'float32')]
        self.coarse_matching = SuperPointMatching(cfg.coarse_matching.num_correspondences,
                                                  cfg.coarse_matching.dual_normalization)
        f = cfg.fine_matching
        self.fine_matching = LocalGlobalRegistration(f.topk, f.acceptance_radius, mutual=f.mutual,
                                                     confidence_threshold=f.confidence_threshold,
                                                     use_dustbin=f.use_dustbin, use_global_score=f.use_global_score,
                                                     correspondence_threshold=f.correspondence_threshold,
                                                     correspondence_limit=f.correspondence_limit,
                                                     num_refinement_steps=f.num_refinement_steps)
        self.optimal_transport = LearnableLogOptimalTransport(cfg.model.num_sinkhorn_iterations)
        if cfg.variant.endswith('kitti'):
            # The reference's KITTI model always constructs its rotation-supervision and anchor-matching heads
            # (experiments/se3eti.kitti/model.py:82-87) although the forward only reaches them with supervise_rotation /
            # anchor_matching (both off in its config).  They are carried as parameter holders so that a reference checkpoint
            # loads with strict=True; nothing here evaluates them.
            from .modules.transformer.permutation_invariant import PermutationInvariantLayer
            from .modules.transformer.rotation_supervision import RotationAttentionLayer
            self.rotation_supervision = RotationAttentionLayer(g.output_dim, g.num_heads)
            self.permutation_invariant = PermutationInvariantLayer(cfg.epn.kanchor, g.output_dim)
        self._tls = threading.local()       # per-thread pinned scratch (pairs may be processed by several host threads)
        self.packed_inference = True        # inference of one pair through se3et_amd.batched.forward_pairs (False: the per-module path)
        self.stage_hook = None              # optional callable invoked between backbone and transformer (pipelined drivers)
        self.emit_ground_truth = False      # inference: also emit gt_node_corr_indices / _overlaps when data_dict has 'transform'

    # Load paths drop the derived-weight caches of se3et_amd.ops (f16 pieces, stacked weights): load_state_dict copies in place (it bumps
    # the version counters anyway), `.to()` / `.float()` / `.half()` go through _apply and may swap a Parameter's storage.
    def load_state_dict(self, *args, **kwargs):
        from . import ops as _ops
        _ops.clear_weight_caches()
        return super().load_state_dict(*args, **kwargs)

    def _apply(self, fn, *args, **kwargs):
        from . import ops as _ops
        _ops.clear_weight_caches()
        return super()._apply(fn, *args, **kwargs)

    def forward(self, data_dict, with_registration=True, train=False, targets=None, rng=None):
        """`train=False`: INFERENCE forward (no autograd), below.  `train=True`: the training forward of the reference
        (experiments/se3ete.3dmatch/model.py:110-131,172-178) with autograd through the HIP ops (se3et_amd.autograd): ground-truth
        superpoint correspondences from data_dict['transform'], fine matching on (at most 128 randomly selected) ground-truth
        patch pairs -- `targets` = (ref_indices, src_indices) overrides the random selection, `rng` seeds it."""
        if train:
            return self._forward(data_dict, with_registration, True, targets, rng)
        if (self.packed_inference and self.stage_hook is None and getattr(self.transformer.transformer, 'layer_tap', None) is None
                and not (self.emit_ground_truth and 'transform' in data_dict) and len(data_dict['lengths'][0]) == 2):
            # the packed-row kernels of the several-pairs forward with ONE pair: same outputs (tests/test_gpu_model.py runs the golden
            # fixtures through both), 7 % less wall time per pair than the per-module path below
            from .batched import forward_pairs
            return forward_pairs(self, data_dict, with_registration)[0]
        with torch.no_grad():
            return self._forward(data_dict, with_registration, False, None, None)

    def _forward(self, data_dict, with_registration, train, targets, rng):
        """INFERENCE forward of one pair (runs under torch.no_grad: the kernels have no autograd; the training step lives in
        se3et_amd.training).  data_dict: output of se3et_amd.data (GPU tensors, host lengths).  Output keys are the reference's
        (experiments/se3ete.3dmatch/model.py:79-227) except the ground-truth keys gt_node_corr_indices / gt_node_corr_overlaps,
        which need `transform` and are produced by se3et_amd.training.node_correspondences."""
        out = {}
        feats = data_dict['features']
        n_c, n_f = int(data_dict['lengths'][-1][0]), int(data_dict['lengths'][1][0])
        points_c, points_f = data_dict['points'][-1], data_dict['points'][1]
        ref_c, src_c, ref_f, src_f = points_c[:n_c], points_c[n_c:], points_f[:n_f], points_f[n_f:]
        n_0 = int(data_dict['lengths'][0][0])
        out.update(ref_points_c=ref_c, src_points_c=src_c, ref_points_f=ref_f, src_points_f=src_f,
                   ref_points=data_dict['points'][0][:n_0], src_points=data_dict['points'][0][n_0:])

        _, ref_nm, ref_knn, ref_km = point_to_node_partition(ref_f, ref_c, self.num_points_in_patch)
        _, src_nm, src_knn, src_km = point_to_node_partition(src_f, src_c, self.num_points_in_patch)
        ref_knn_pts = SF.gather_rows_padded(ref_f, ref_knn)
        src_knn_pts = SF.gather_rows_padded(src_f, src_knn)
        if train or (self.emit_ground_truth and 'transform' in data_dict):
            # ground-truth superpoint correspondences (the reference computes them in every forward; they need the transform)
            from .training import node_correspondences
            gi, go = node_correspondences(ref_c, src_c, ref_knn_pts, src_knn_pts, data_dict['transform'],
                                          self.cfg.model.ground_truth_matching_radius, ref_nm, src_nm, ref_km, src_km)
            out['gt_node_corr_indices'], out['gt_node_corr_overlaps'] = gi, go
        # number of non-empty nodes, fetched asynchronously (read only after the transformer, when it has long arrived)
        valid_host = getattr(self._tls, 'valid_host', None)
        if valid_host is None:
            valid_host = self._tls.valid_host = torch.empty(2, dtype=torch.int64).pin_memory()
        valid_host.copy_(torch.stack((ref_nm.sum(), src_nm.sum())), non_blocking=True)
        valid_event = torch.cuda.Event()
        valid_event.record()

        feats_list = self.backbone(feats, data_dict)
        feats_c, feats_f = feats_list[-1], feats_list[0]
        out['feats_c'], out['feats_f'] = feats_c, feats_f
        if self.stage_hook is not None:
            self.stage_hook()

        r, s, _, _, _, _ = self.transformer(ref_c.unsqueeze(0), src_c.unsqueeze(0), feats_c[:n_c].unsqueeze(0),
                                            feats_c[n_c:].unsqueeze(0))
        r, s = F.normalize(r.squeeze(0), p=2, dim=1), F.normalize(s.squeeze(0), p=2, dim=1)
        out['ref_feats_c'], out['src_feats_c'] = r, s
        out['ref_feats_f'], out['src_feats_f'] = feats_f[:n_f], feats_f[n_f:]

        valid_event.synchronize()
        all_valid = valid_host.tolist() == [ref_c.shape[0], src_c.shape[0]]
        ri, si, node_scores = self.coarse_matching(r.detach(), s.detach(), ref_nm, src_nm, all_valid=all_valid)
        out['ref_node_corr_indices'], out['src_node_corr_indices'], out['node_corr_scores'] = ri, si, node_scores
        if train:          # fine matching on ground-truth patch pairs (model.py:172-178, superpoint_target.py)
            from .training import select_targets
            cm = self.cfg.coarse_matching
            if targets is not None:
                ri, si = targets[0].to(ri.device), targets[1].to(ri.device)
                node_scores = torch.ones(ri.shape[0], device=ri.device)
            else:
                ri, si, node_scores = select_targets(out['gt_node_corr_indices'], out['gt_node_corr_overlaps'], cm.num_targets,
                                                     cm.overlap_threshold, rng)

        ref_ck, src_ck = ref_knn[ri], src_knn[si]
        ref_cm, src_cm = ref_km[ri], src_km[si]
        ref_cp, src_cp = ref_knn_pts[ri], src_knn_pts[si]
        rk = SF.gather_rows_padded(feats_f[:n_f], ref_ck)
        sk = SF.gather_rows_padded(feats_f[n_f:], src_ck)
        out.update(ref_node_corr_knn_points=ref_cp, src_node_corr_knn_points=src_cp, ref_node_corr_knn_masks=ref_cm,
                   src_node_corr_knn_masks=src_cm)
        scores = torch.einsum('bnd,bmd->bnm', rk, sk) / feats_f.shape[1] ** 0.5
        scores = self.optimal_transport(scores, ref_cm, src_cm)
        out['matching_scores'] = scores
        if with_registration:
            with torch.no_grad():
                rc, sc, cs, T = self.fine_matching(ref_cp, src_cp, ref_cm, src_cm, scores.detach()[:, :-1, :-1], node_scores)
            out.update(ref_corr_points=rc, src_corr_points=sc, corr_scores=cs, estimated_transform=T)
        return out


def create_model(cfg):
    return SE3ET(cfg)


def load_synthetic_weights(model, seed=7):
    """Name-keyed deterministic weights (se3et_amd.synthetic.synth_tensor) for every learned parameter; the constant
    tables (kernel points, anchors, permutation indices, div_term, Wigner tables) are left as constructed."""
    from .synthetic import synth_tensor
    sd = model.state_dict()
    for k, v in sd.items():
        leaf = k.rsplit('.', 1)[-1]
        if leaf in ('weight', 'bias', 'weights', 'alpha') and v.dtype == torch.float32 and 'anchors' not in k:
            sd[k] = torch.from_numpy(np.asarray(synth_tensor(k, tuple(v.shape), seed), dtype=np.float32).reshape(tuple(v.shape))).to(v.device)
    model.load_state_dict(sd)
    return model
