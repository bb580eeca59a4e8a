#!/usr/bin/env python3
"""Audit of asm register loads in a kernel's device assembly (hipcc --cuda-device-only -S):

    pass_entry_audit.py <file.s> <substring of the kernel's mangled name>

Every run of global_load_dword / global_load_dwordx4 register loads up to the next s_waitcnt vmcnt(0) is one entry: the
VGPRs the loads write are collected, and every instruction between a load and the wait that names one of them is
reported as BAD (a read or a copy of a register whose data has not landed).  The first entry is printed in full.
"""
import re,sys
f,pat=sys.argv[1],sys.argv[2]
lines=[];on=False
for l in open(f):
    m=re.match(r'^(_Z\w+):',l)
    if m: on = pat in m.group(1)
    if on:
        if l.startswith('.Lfunc_end'): break
        lines.append(l.rstrip('\n'))
def regs(tok):
    out=set()
    for m in re.finditer(r'\bv\[(\d+):(\d+)\]|\bv(\d+)\b',tok):
        if m.group(3): out.add(int(m.group(3)))
        else: out.update(range(int(m.group(1)),int(m.group(2))+1))
    return out
i=0;entry=0
while i<len(lines):
    s=lines[i].split(';')[0].strip()
    if re.match(r'global_load_dword(x4)?\s',s):
        # a pass entry: from here to the next s_waitcnt vmcnt(0)
        j=i
        while 's_waitcnt vmcnt(0)' not in lines[j]: j+=1
        entry+=1
        loaded=set();bad=[]
        for k in range(i,j+1):
            t=lines[k].split(';')[0].strip()
            if not t or t.startswith('.'): continue
            if re.match(r'global_load_dword(x4)?\s',t):
                ops=t.split(None,1)[1].split(',')
                used=regs(','.join(ops[1:])); 
                if used&loaded: bad.append(t)
                loaded|=regs(ops[0])
            elif regs(t)&loaded: bad.append(t)
        print("== pass entry %d of %s: lines %d..%d of the kernel, %d loaded VGPRs, %d instructions that name one of them before the wait"%(entry,pat,i,j,len(loaded),len(bad)))
        for b in bad: print("   BAD",b)
        if entry==1:
            for k in range(max(i-3,0),min(j+14,len(lines))): print(lines[k])
        i=j
    i+=1
