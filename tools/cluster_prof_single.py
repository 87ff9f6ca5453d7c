#!/usr/bin/env python3
"""The single cluster_embeddings call of tools/cluster_bench.py, three times, for a kernel trace:
  rocprofv3 --kernel-trace --stats -d OUT -- python tools/cluster_prof_single.py"""
import cluster_bench as cb
import torch

E = torch.from_numpy(cb.embeddings()).cuda()
for _ in range(3):
    cb.cl.cluster_embeddings(E, cb.K, cb.SEED)
torch.cuda.synchronize()
