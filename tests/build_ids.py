"""The recorded build ids of the nine libraries and what tests/test_build_identity.py expects of each.

IDS: source_hash() of every library under the compiler that profiles/r05_build_id.txt records.  A change that alters a
library's id updates exactly one row here (and, for "hip", means the committed profiles no longer describe the build)."""
from collections import namedtuple

IDS = {
    "hip": "3d06e0f4bcfa769a89bb163e",
    "critic": "1afdcabad09cc0d419a8d9a5",
    "statewise": "e6d760b1dbf2d5195c1247e0",
    "safelayer": "de39af70500c88f6609d39c8",
    "usl": "1175e0847c1bddf1d90b8286",
    "lpg": "e196100c68b94afce543fb6f",
    "episode": "2ac1225ff7d697761c70297a",
    "mathprobe": "1500249652e842aae76b306b",
    "epstats": "8ca027aecb951893fa8482eb",
}

# prefix: of the C symbols; macro: carries the id into the library; step_args: the binding's mirror of gx?_step_args;
# protos: functions the header declares under the prefix; values: its enumerators (the four statuses among them);
# extra: the binding's symbol set declared under the library's full name (guardx_<key>_...)
Row = namedtuple("Row", "prefix macro step_args protos values extra")
ROWS = {
    "hip": Row("gx", "GX_BUILD_ID", None, 50, None, None),
    "critic": Row("gxc", "GXC_BUILD_ID", None, 5, 4, None),
    "statewise": Row("gxs", "GXS_BUILD_ID", "GxsStepArgs", 7, 4, None),
    "safelayer": Row("gxl", "GXL_BUILD_ID", "GxlStepArgs", 8, 4, "EPISODE_SYMBOLS"),
    "usl": Row("gxu", "GXU_BUILD_ID", "GxuStepArgs", 9, 4, "EPISODE_SYMBOLS"),
    "lpg": Row("gxp", "GXP_BUILD_ID", "GxpStepArgs", 9, 4, "EPISODE_SYMBOLS"),
    "episode": Row("gxe", "GXE_BUILD_ID", "GxeStepArgs", 10, 4, "COLS_SYMBOLS"),
    "mathprobe": Row("gxm", "GXM_BUILD_ID", None, 5, 4 + 12 + 5, None),
    "epstats": Row("gxt", "GXT_BUILD_ID", None, 5, 4 + 8, None),
}
