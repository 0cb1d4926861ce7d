"""The ctypes layouts of trexhip_prefilter_params / trexhip_prefilter_tables (trex_amd/capi.py) against sizeof / offsetof of the C structs in
include/trexhip.h, through a compiled probe."""
import ctypes as C
import os
import subprocess
from trex_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_prefilter_struct_layouts_match_header(tmp_path):
    structs = {"trexhip_prefilter_params": capi.PrefilterParams, "trexhip_prefilter_tables": capi.PrefilterTables}
    exprs, want = [], []
    for cname, cls in structs.items():
        exprs.append("sizeof(%s)" % cname)
        want.append(C.sizeof(cls))
        for field, _ in cls._fields_:
            exprs.append("offsetof(%s,%s)" % (cname, field))
            want.append(getattr(cls, field).offset)
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "trexhip.h"\nint main(void){size_t v[]={%s};'
                   'for(unsigned i=0;i<sizeof v/sizeof v[0];++i)printf("%%zu ",v[i]);return 0;}\n' % ",".join(exprs))
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == want, list(zip(exprs, got, want))
