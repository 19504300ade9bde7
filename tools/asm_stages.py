#!/usr/bin/env python3
"""Instruction mix between consecutive s_barrier instructions of one kernel (in program order): asm_stages.py file.s kernel-substring"""
import collections, os, re, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scream_amd.asm_check import kernels
key = sys.argv[2]
body = next(b for n, b in kernels(sys.argv[1]) if key in n)[1:]
segs = []; c = collections.Counter(); lab = 'entry'
for l in body:
    t = l.strip()
    if not t or t.startswith(';'): continue
    if re.match(r'^\.LBB\d+_\d+:', t):
        c['labels'] += 1; lab = t.split(':')[0]; continue
    op = t.split()[0]
    if op == 's_barrier':
        segs.append((lab, c)); c = collections.Counter(); continue
    if op.startswith('v_mfma'): c['mfma'] += 1
    elif 'accvgpr' in op: c['acc_mov'] += 1
    elif op.startswith('v_pk_'): c['valu_pk'] += 1
    elif op.startswith(('v_exp', 'v_rcp', 'v_rsq', 'v_sqrt', 'v_log')): c['trans'] += 1
    elif op.startswith('v_'): c['valu'] += 1
    elif op.startswith('ds_read') or op.startswith('ds_load'): c['ds_rd'] += 1
    elif op.startswith('ds_'): c['ds_wr'] += 1
    elif op.startswith('global_load_lds'): c['dma'] += 1
    elif op.startswith('global_load'): c['gld'] += 1
    elif op.startswith('global_store'): c['gst'] += 1
    elif op.startswith('scratch_'): c['scratch'] += 1
    elif op == 's_nop': c['nop'] += 1
segs.append((lab, c))
keys = ['mfma', 'valu', 'valu_pk', 'trans', 'acc_mov', 'ds_rd', 'ds_wr', 'dma', 'gld', 'gst', 'nop', 'scratch', 'labels']
print('%-4s %-10s ' % ('#', 'label') + ' '.join('%7s' % k for k in keys))
for i, (lab, c) in enumerate(segs):
    print('%-4d %-10s ' % (i, lab) + ' '.join('%7d' % c[k] for k in keys))
