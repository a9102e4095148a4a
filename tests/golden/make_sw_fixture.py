"""Build tests/golden/sw_panel.npz from the reference's spreadsheet (run in the build container only).

    python tests/golden/make_sw_fixture.py [/root/reference]

The fixture is the `:All` Stock-Watson panel exactly as `readin_data(md, qd, BiWeight(100), :All)` returns
it (readin_functions.jl:355-382; constants Stock_Watson.ipynb:143-144, 180): `bpdata` 224 x 207 (NaN =
missing), `inclcode`, `bpcatcode`, `bpnamevec`, `calvec`.  The `:Real` panel of Stock_Watson.ipynb:160 is
the column subset floor(bpcatcode) in {1,2,3,5} (readin_functions.jl:254) - asserted here and in
tests/test_oracle_sw.py.  `/root/reference` does not exist on the GPU box, so tests read this file.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import sw_panel as sp  # noqa: E402

ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
xlsx = os.path.join(ref, "data", "hom_fac_1.xlsx")
dA = sp.readin_data(xlsx, "All")
dR = sp.readin_data(xlsx, "Real")
keep = np.isin(np.floor(dA["bpcatcode"]), [1, 2, 3, 5])
assert np.array_equal(dA["bpdata"][:, keep], dR["bpdata"], equal_nan=True)
assert np.array_equal(dA["inclcode"][keep], dR["inclcode"])
assert dA["bpdata"].shape == (224, 207) and dR["bpdata"].shape == (224, 86)
out = os.path.join(ROOT, "tests", "golden", "sw_panel.npz")
np.savez_compressed(out, bpdata=dA["bpdata"], inclcode=dA["inclcode"].astype(np.int64),
                    bpcatcode=dA["bpcatcode"], bpnamevec=np.array(dA["bpnamevec"]), calvec=dA["calvec"])
print(out, os.path.getsize(out), "bytes")

# tests/golden/hom_fac_1_sheets.xlsx: the two sheets readin_data reads ("Monthly", "Quarterly"), cell values only (no formulas,
# styles or other sheets; the spreadsheet itself is over the size limit of a committed file), LZMA-compressed.  It lets
# tests/test_oracle_sw.py run the restated ingestion from the spreadsheet's cells without the reference.
import xml.etree.ElementTree as ET  # noqa: E402
import zipfile  # noqa: E402

NS = "http://schemas.openxmlformats.org/spreadsheetml/2006/main"
RNS = "http://schemas.openxmlformats.org/officeDocument/2006/relationships"
esc = lambda s: s.replace("&", "&amp;").replace("<", "&lt;").replace(">", "&gt;")


def values_only(xml):
    rows = []
    for row in ET.fromstring(xml).iter(f"{{{NS}}}row"):
        cells = []
        for c in row.iter(f"{{{NS}}}c"):
            v, t = c.find(f"{{{NS}}}v"), c.get("t", "n")
            if v is not None and v.text not in (None, ""):
                cells.append(f'<c r="{c.get("r")}"' + ("" if t == "n" else f' t="{t}"') + f"><v>{esc(v.text)}</v></c>")
        if cells:
            rows.append(f'<row r="{row.get("r")}">' + "".join(cells) + "</row>")
    return f'<?xml version="1.0" encoding="UTF-8" standalone="yes"?>\n<worksheet xmlns="{NS}"><sheetData>' + "\n".join(rows) + "</sheetData></worksheet>"


with zipfile.ZipFile(xlsx) as z:
    wb = ET.fromstring(z.read("xl/workbook.xml"))
    rels = {r.get("Id"): r.get("Target") for r in ET.fromstring(z.read("xl/_rels/workbook.xml.rels"))}
    targets = {s.get("name"): rels[s.get(f"{{{RNS}}}id")] for s in wb.iter(f"{{{NS}}}sheet")}
    sheets = {name: values_only(z.read("xl/" + targets[name])) for name in ("Monthly", "Quarterly")}
    shared = z.read("xl/sharedStrings.xml")
small = os.path.join(ROOT, "tests", "golden", "hom_fac_1_sheets.xlsx")
with zipfile.ZipFile(small, "w", zipfile.ZIP_LZMA) as z:
    z.writestr("xl/workbook.xml", f'<?xml version="1.0" encoding="UTF-8" standalone="yes"?>\n<workbook xmlns="{NS}" xmlns:r="{RNS}"><sheets>'
               '<sheet name="Monthly" sheetId="1" r:id="rId1"/><sheet name="Quarterly" sheetId="2" r:id="rId2"/></sheets></workbook>')
    z.writestr("xl/_rels/workbook.xml.rels", '<?xml version="1.0" encoding="UTF-8" standalone="yes"?>\n'
               '<Relationships xmlns="http://schemas.openxmlformats.org/package/2006/relationships">'
               f'<Relationship Id="rId1" Type="{RNS}/worksheet" Target="worksheets/sheet1.xml"/>'
               f'<Relationship Id="rId2" Type="{RNS}/worksheet" Target="worksheets/sheet2.xml"/>'
               f'<Relationship Id="rId3" Type="{RNS}/sharedStrings" Target="sharedStrings.xml"/></Relationships>')
    z.writestr("xl/worksheets/sheet1.xml", sheets["Monthly"])
    z.writestr("xl/worksheets/sheet2.xml", sheets["Quarterly"])
    z.writestr("xl/sharedStrings.xml", shared)
for kind, d in (("All", dA), ("Real", dR)):
    s = sp.readin_data(small, kind)
    assert np.array_equal(s["bpdata"], d["bpdata"], equal_nan=True) and s["bpnamevec"] == d["bpnamevec"]
    assert np.array_equal(s["inclcode"], d["inclcode"])
print(small, os.path.getsize(small), "bytes")
